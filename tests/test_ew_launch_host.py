"""Host checks (no GPU) behind tests/test_ew_launches.py: the BatchNorm / resize launch lists of the benchmark's pyramids, the
BatchNorm launch plan (fused path or three launches, nsplit, vector width) the library picks for each of them, the float64
references of tests/ew_ref.py against torch autograd over the oracle, and the power of their per-element error bounds."""
import pytest
import torch
import torch.nn.functional as F

import conv_ref as R
import ew_ref as E
from helpers import RTOL, assert_close
from oracle import hpvg_oracle as O


@pytest.fixture(scope="module")
def lib():
    import hp_vae_gan_amd  # noqa: F401
    from hp_vae_gan_amd import lib as hplib
    return hplib.load()


def test_launch_lists():
    """27 distinct level shapes x (B, groups) = (2, 1), (4, 2), (1, 1); the level-to-level resizes of the three pyramids;
    the baselines critic's padded video8 volumes."""
    shapes = R.level_shapes()
    bn = E.bn_launches()
    assert len(bn) == 27 * 3 and len(set((l[2], l[3]) for l in bn)) == len(bn)
    assert set(E.BN_PLANS) == set(s for sh in shapes.values() for s in sh)
    rs = E.resize_launches()
    assert len(rs) == sum(len(sh) - 1 for sh in shapes.values()) == 9 + 7 + 9
    assert all(len(a) == len(b) and all(o >= i for i, o in zip(a, b)) for _, _, a, b in rs)   # every transition upsamples
    assert set(E.padded_shapes()) == set(E.BN2_PLANS) and max(E.BN2_PLANS) == (27, 158, 270)


def test_bn_plan_of_every_launch(lib):
    """hpvg_bn_plan returns the committed table for every BatchNorm launch; the table holds both paths, all three vector
    widths, and groups = 2 on both paths."""
    bad = []
    for _, _, sp, B, groups in E.bn_launches():
        got, want = E.bn_plan_of(lib, B, E.spatial(sp), groups), E.expected_plan(sp, B, groups)
        if got != want:
            bad.append("%s B=%d groups=%d: (fused, nsplit, V) %s, table %s" % (sp, B, groups, got, want))
    for sp, want in E.BN2_PLANS.items():
        got = E.bn_plan_of(lib, 2, E.spatial(sp), 1)
        if got != want:
            bad.append("bwd2 %s B=2: %s, table %s" % (sp, got, want))
    assert not bad, "\n".join(bad)
    plans = [(E.expected_plan(sp, B, g), g) for _, _, sp, B, g in E.bn_launches()]
    assert {p[2] for p, _ in plans} == {1, 2, 4}
    assert {p[0] for p, g in plans if g == 2} == {0, 1} and {p[0] for p, g in plans if g == 1} == {0, 1}
    # the size rule itself: fused up to 2^25 elements of the whole batch
    assert E.bn_plan_of(lib, 2, 1 << 18, 1)[0] == 1 and E.bn_plan_of(lib, 2, (1 << 18) + 1, 1)[0] == 0
    import ctypes
    out = (ctypes.c_int * 3)()
    assert lib.hpvg_bn_plan(3, 64, 8, 2, out) != 0          # B not divisible by groups


def _data(B, C, sp, seed, offset=1.0):
    g = torch.Generator().manual_seed(seed)
    r = torch.randn(B, C, *sp, generator=g, dtype=torch.float64) * (0.5 + torch.rand(1, C, *([1] * len(sp)), generator=g, dtype=torch.float64))
    r = r + offset * (torch.rand(1, C, *([1] * len(sp)), generator=g, dtype=torch.float64) * 2 - 1)
    gamma = 1 + 0.3 * torch.randn(C, generator=g, dtype=torch.float64)
    beta = 0.3 * torch.randn(C, generator=g, dtype=torch.float64)
    rm = 0.1 * torch.randn(C, generator=g, dtype=torch.float64)
    rv = 1 + 0.2 * torch.rand(C, generator=g, dtype=torch.float64)
    dh = torch.randn(B, C, *sp, generator=g, dtype=torch.float64)
    G = torch.randn(B, C, *sp, generator=g, dtype=torch.float64)
    return r, gamma, beta, rm, rv, dh, G


def _close(got, ref, A, what, tol=1e-12):
    err = float((got.double() - ref.double()).abs().max())
    scale = float(A.double().max())
    assert err <= tol * scale, "%s: %.3e > %.0e * %.3e" % (what, err, tol, scale)


# S = 6 * 5 = 30 (V = 2), 7 * 3 = 21 (V = 1), 4 * 6 (V = 4), T = 1 and H or W = 1
BN_SMALL = [((2, 5, 3), 4, 2), ((3, 7), 2, 1), ((1, 7, 3), 4, 2), ((2, 1, 6), 2, 1), ((4, 6), 4, 2), ((1, 1, 9), 2, 2)]


@pytest.mark.parametrize("sp,B,groups", BN_SMALL)
@pytest.mark.parametrize("lrelu", [True, False])
def test_bn_reference_against_autograd(sp, B, groups, lrelu):
    """bn_fwd64 / bn_bwd64 against O.batch_norm_train (forward, running buffers) and torch autograd of float64 train-mode
    F.batch_norm (backward; the oracle's own backward rounds its sums to fp32), one group after the other, within 1e-12 of
    the error scale.  The direct-slot form adds the preset gradient."""
    C = 5
    r, gamma, beta, rm, rv, dh, _ = _data(B, C, sp, seed=B * 100 + len(sp) * 10 + groups)
    ref = E.bn_fwd64(r, gamma, beta, rm, rv, groups=groups, lrelu=lrelu)
    Bg = B // groups
    rm_o, rv_o = rm.clone(), rv.clone()
    rm_t, rv_t = rm.clone(), rv.clone()
    outs, dr_parts, dg, db = [], [], 0, 0
    stats = torch.empty(groups, 4, C, dtype=torch.float64)
    for k in range(groups):
        xk = r[k * Bg:(k + 1) * Bg]
        y = O.batch_norm_train(xk, gamma, beta, rm_o, rv_o)
        outs.append(O.leaky_relu(y) if lrelu else y)
        xr, gr, br = xk.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
        yt = F.batch_norm(xr, rm_t, rv_t, gr, br, training=True, momentum=E.BN_MOMENTUM, eps=E.BN_EPS)
        if lrelu:
            yt = F.leaky_relu(yt, E.SLOPE)
        a, b_, c = torch.autograd.grad(yt, [xr, gr, br], dh[k * Bg:(k + 1) * Bg])
        dr_parts.append(a)
        dg, db = dg + b_, db + c
        for j, key in enumerate(("mean", "invstd", "scale", "shift")):
            stats[k, j] = ref[key][0][k]
    h, hA = ref["h"]
    _close(h, torch.cat(outs), hA, "h")
    _close(ref["rm"][0], rm_o, ref["rm"][1], "running_mean")
    _close(ref["rv"][0], rv_o, ref["rv"][1], "running_var")
    _close(ref["rm"][0], rm_t, ref["rm"][1], "running_mean (F.batch_norm)")
    _close(ref["rv"][0], rv_t, ref["rv"][1], "running_var (F.batch_norm)")
    x = r.reshape(groups, Bg, C, -1)
    mean = x.mean(dim=(1, 3))
    _close(ref["mean"][0], mean, ref["mean"][1], "mean")
    _close(ref["invstd"][0], 1 / (x.var(dim=(1, 3), unbiased=False) + E.BN_EPS).sqrt(), ref["invstd"][1], "invstd")
    _close(ref["shift"][0], beta - mean * ref["scale"][0], ref["shift"][1], "shift")
    bwd = E.bn_bwd64(dh, r, stats, groups=groups, lrelu=lrelu)
    _close(bwd["dr"][0], torch.cat(dr_parts), bwd["dr"][1], "dr")
    _close(bwd["dgamma"][0], dg, bwd["dgamma"][1], "dgamma")
    _close(bwd["dbeta"][0], db, bwd["dbeta"][1], "dbeta")
    base_g, base_b = torch.randn(C, dtype=torch.float64), torch.randn(C, dtype=torch.float64)
    slot = E.bn_bwd64(dh, r, stats, groups=groups, lrelu=lrelu, base_gamma=base_g, base_beta=base_b)
    _close(slot["dgamma"][0], base_g + dg, slot["dgamma"][1], "dgamma, direct slot")
    _close(slot["dbeta"][0], base_b + db, slot["dbeta"][1], "dbeta, direct slot")
    assert bool((slot["dbeta"][1] >= bwd["dbeta"][1]).all()) and torch.equal(slot["dr"][0], bwd["dr"][0])


@pytest.mark.parametrize("sp,B", [((2, 5, 3), 2), ((3, 7), 2), ((1, 7, 3), 1), ((2, 1, 6), 3)])
@pytest.mark.parametrize("lrelu", [True, False])
def test_bn_second_order_reference_against_autograd(sp, B, lrelu):
    """bn_bwd2_64 (the kernel comment's closed form) against double autograd of lrelu?(batch_norm(r)) in float64 - torch's
    F.batch_norm and O.batch_norm_train's differentiable backward - within 1e-12 of A (the oracle's fp32-rounded sums:
    1e-6)."""
    C = 4
    r, gamma, beta, rm, rv, dh, G = _data(B, C, sp, seed=7 + B + len(sp))
    ref = E.bn_fwd64(r, gamma, beta, rm, rv, lrelu=lrelu)
    stats = torch.stack([ref[k][0] for k in ("mean", "invstd", "scale", "shift")], dim=1)
    got = E.bn_bwd2_64(dh, G, r, stats, lrelu=lrelu)
    for name, bn, tol in (("F.batch_norm", lambda x, g, b: F.batch_norm(x, None, None, g, b, training=True, eps=E.BN_EPS), 1e-12),
                          ("oracle", lambda x, g, b: O.batch_norm_train(x, g, b), 1e-6)):
        xr, gr, dhr = r.clone().requires_grad_(True), gamma.clone().requires_grad_(True), dh.clone().requires_grad_(True)
        y = bn(xr, gr, beta)
        if lrelu:
            y = O.leaky_relu(y)
        (dr,) = torch.autograd.grad(y, [xr], dhr, create_graph=True)
        g_dh, g_r, g_g = torch.autograd.grad((dr * G).sum(), [dhr, xr, gr])
        _close(got["g_dh"][0], g_dh, got["g_dh"][1], name + " g_dh", tol)
        _close(got["g_r"][0], g_r, got["g_r"][1], name + " g_r", tol)
        _close(got["g_gamma"][0], g_g, got["g_gamma"][1], name + " g_gamma", tol)


@pytest.mark.parametrize("ins,outs", [((4, 18, 33), (4, 23, 41)), ((5, 45, 81), (5, 57, 102)), ((7, 114, 204), (13, 144, 256)),
                                      ((1, 3, 5), (1, 7, 5)), ((2, 1, 4), (3, 1, 9)), ((24, 33), (30, 41)), ((5, 1), (9, 1))])
def test_resize_reference_against_autograd(ins, outs):
    """resize64 / resize_bwd64 against float64 F.interpolate(align_corners=True) and its autograd (the adjoint), within
    1e-12 of A; the oracle's resize (fp32 coordinates, as the kernel) stays within the coordinate bound TAU * A."""
    g = torch.Generator().manual_seed(sum(ins) + sum(outs))
    C = 2
    x = torch.randn(1, C, *ins, generator=g, dtype=torch.float64)
    dy = torch.randn(1, C, *outs, generator=g, dtype=torch.float64)
    dy2 = torch.randn(1, C, *outs, generator=g, dtype=torch.float64)
    noise = torch.randn(1, C, *outs, generator=g, dtype=torch.float64)
    mode = "trilinear" if len(ins) == 3 else "bilinear"
    xr = x.clone().requires_grad_(True)
    yt = F.interpolate(xr, size=outs, mode=mode, align_corners=True)
    (dxt,) = torch.autograd.grad(yt, [xr], dy + dy2)
    y, A, yn, ynA = E.resize64(x, outs, noise, 0.3)
    _close(y, yt, A, "resize")
    _close(yn, yt + 0.3 * noise, ynA, "resize + noise")
    dx, dA = E.resize_bwd64(dy, ins, dy2)
    _close(dx, dxt, dA, "adjoint")
    y_o = O.resize_linear_ac(x, outs)
    assert R.err_ratio(y_o, y, A)[0] <= E.TAU
    # A also bounds the fp32 products: resize(|x|) <= A
    assert bool((E.resize64(x.abs(), outs)[0] <= A * (1 + 1e-12)).all())


def test_gp_and_loss_references_against_autograd():
    """gp64, mse64, kl64, mean_scaled64, sqsum64 and their gradients against float64 autograd of the oracle's formulas."""
    g = torch.Generator().manual_seed(5)
    gr = torch.randn(2, 3, 3, 4, 5, generator=g, dtype=torch.float64)
    gr[1, :, 0, 0, 0] = 0                                                     # a voxel with a zero norm: zero gradient
    gq = gr.clone().requires_grad_(True)
    P = 0.1 * ((gq.norm(2, dim=1) - 1) ** 2).mean()
    (dP,) = torch.autograd.grad(P, [gq], torch.tensor(0.7, dtype=torch.float64))
    p, pA = E.gp64(gr, 0.1)
    _close(p, P.detach(), pA, "gp")
    dg, dgA = E.gp_bwd64(0.7, gr, 0.1)
    _close(dg, torch.nan_to_num(dP), dgA, "gp backward")
    assert float(dg[1, :, 0, 0, 0].abs().max()) == 0 and float(dgA[1, :, 0, 0, 0].max()) == 0

    a, b = torch.randn(2, 3, 4, 5, generator=g, dtype=torch.float64), torch.randn(2, 3, 4, 5, generator=g, dtype=torch.float64)
    aq = a.clone().requires_grad_(True)
    m = O.mse(aq, b)
    (da,) = torch.autograd.grad(m, [aq], torch.tensor(1.3, dtype=torch.float64))
    v, vA = E.mse64(a, b)
    _close(v, m.detach(), vA, "mse")
    d, dA = E.mse_bwd64(1.3, a, b)
    _close(d, da, dA, "mse backward")

    mu, lv = a.clone().requires_grad_(True), (0.5 * b).clone().requires_grad_(True)
    k = O.kl_criterion(mu, lv)
    dmu, dlv = torch.autograd.grad(k, [mu, lv], torch.tensor(0.9, dtype=torch.float64))
    v, vA = E.kl64(a, 0.5 * b)
    _close(v, k.detach(), vA, "kl")
    (m1, m1A), (l1, l1A) = E.kl_bwd64(0.9, a, 0.5 * b)
    _close(m1, dmu, m1A, "kl dmu")
    _close(l1, dlv, l1A, "kl dlogvar")

    v, vA = E.mean_scaled64(a, -1.0)
    _close(v, -a.mean(), vA, "mean-scaled")
    v, vA = E.sqsum64(a)
    _close(v, (a * a).sum(), vA, "sqsum")


# ------------------------------------------------------------------------------------------------ checker power
def _level0(B=4, groups=2, seed=11):
    """The first video level's BatchNorm at B = 4 (the merged pass, groups = 2), float64 on CPU."""
    sp = R.level_shapes()["video"][0]
    r, gamma, beta, rm, rv, dh, _ = _data(B, E.BN_C, sp, seed=seed, offset=0.5)
    return sp, r.float(), gamma.float(), beta.float(), rm.float(), rv.float(), dh.float()


def _fp32_bn(r, gamma, beta, groups, lrelu=True, stats_of=None, drop_split=None):
    """A BatchNorm forward computed in fp32 from float64 statistics - the arithmetic the kernels do, up to rounding - with
    optional faults: stats_of[k] = the group whose statistics group k uses; drop_split = (nsplit, k): the k-th of nsplit
    chunks of every sample row is missing from the sums (as in bn_stats_partial_kernel's split)."""
    B, C = r.shape[:2]
    x = r.double().reshape(groups, B // groups, C, -1)
    S = x.shape[-1]
    n = torch.ones(S, dtype=torch.float64)
    if drop_split is not None:
        ns, k = drop_split
        chunk = -(-S // ns)
        n[k * chunk:(k + 1) * chunk] = 0
    N = x.shape[1] * S
    mean = (x * n).sum(dim=(1, 3)) / N
    var = ((x * x) * n).sum(dim=(1, 3)) / N - mean * mean
    invstd = 1 / (var + E.BN_EPS).sqrt()
    sel = list(stats_of) if stats_of is not None else list(range(groups))
    sc = (gamma.double() * invstd).float()[sel]
    sh = (beta.double() - mean * gamma.double() * invstd).float()[sel]
    z = r.reshape(groups, B // groups, C, -1) * sc[:, None, :, None] + sh[:, None, :, None]
    return (O.leaky_relu(z) if lrelu else z).reshape(r.shape)


def test_checker_power_batchnorm(lib):
    """At the first video level (4 x 18 x 33, C = 64): a fp32 BatchNorm passes the bound; swapping the two groups'
    statistics, dropping one split partial of the sums, applying the LeakyReLU slope on the wrong side of 0 in the
    backward, or updating the running variance with the biased variance each fail it - and the last passes the suite's
    global-maximum RTOL check."""
    sp, r, gamma, beta, rm, rv, dh = _level0()
    ref = E.bn_fwd64(r, gamma, beta, rm, rv, groups=2)
    h, hA = ref["h"]
    assert R.check(_fp32_bn(r, gamma, beta, 2), h, hA, "fp32 BatchNorm") <= E.TAU
    with pytest.raises(AssertionError, match=r"\|got - ref\| / A"):
        R.check(_fp32_bn(r, gamma, beta, 2, stats_of=(1, 0)), h, hA, "groups' statistics swapped")
    fused, ns, _ = E.bn_plan_of(lib, 4, E.spatial(sp), 2)
    assert fused == 1 and ns == 3
    with pytest.raises(AssertionError, match=r"\|got - ref\| / A"):
        R.check(_fp32_bn(r, gamma, beta, 2, drop_split=(ns, 1)), h, hA, "one split partial dropped")

    # running variance: rv <- 0.9 rv + 0.1 var (biased) instead of the unbiased var, at B = 1 (N = 2376)
    ref1 = E.bn_fwd64(r[:1], gamma, beta, rm, rv, groups=1)
    x = r[:1].double().reshape(1, E.BN_C, -1)
    var_b = x.var(dim=(0, 2), unbiased=False)
    var_u = x.var(dim=(0, 2), unbiased=True)
    rv_good = (0.9 * rv.double() + 0.1 * var_u).float()
    rv_bad = (0.9 * rv.double() + 0.1 * var_b).float()
    rvref, rvA = ref1["rv"]
    assert R.check(rv_good, rvref, rvA, "running var", tau=E.TAU_STAT) <= E.TAU_STAT
    assert_close(rv_bad, rvref, RTOL, "biased running var, global-maximum measure")     # the old measure lets it through
    with pytest.raises(AssertionError, match=r"\|got - ref\| / A"):
        R.check(rv_bad, rvref, rvA, "biased running var", tau=E.TAU_STAT)

    # backward with the slope applied where z >= 0 (mask inverted)
    stats = torch.stack([ref[k][0] for k in ("mean", "invstd", "scale", "shift")], dim=1).float()
    good = E.bn_bwd64(dh, r, stats, groups=2)
    dr, drA = good["dr"]
    assert R.check(dr.float(), dr, drA, "fp32-rounded dr") <= E.TAU
    st = stats.double()
    xs = r.double().reshape(2, 2, E.BN_C, -1)
    z = xs * st[:, 2][:, None, :, None] + st[:, 3][:, None, :, None]
    dh_bad = dh.double().reshape(z.shape) * torch.where(z >= 0, torch.full_like(z, E.SLOPE), torch.ones_like(z))
    bad = E.bn_bwd64(dh_bad.reshape(dh.shape), r, stats, groups=2, lrelu=False)
    with pytest.raises(AssertionError, match=r"\|got - ref\| / A"):
        R.check(bad["dr"][0].float(), dr, drA, "LeakyReLU slope on the wrong side")


def test_checker_power_resize():
    """At the finest video transition (7 x 114 x 204 -> 13 x 144 x 256): the fp32-coordinate resize of the oracle passes
    the bound; a backward gather that misses one output along W (one (o, i) weight of the W axis zeroed) fails it."""
    ins, outs = R.level_shapes()["video"][-2], R.level_shapes()["video"][-1]
    g = torch.Generator().manual_seed(3)
    x = torch.randn(1, 1, *ins, generator=g)
    y, A = E.resize64(x, outs)
    assert R.check(O.resize_linear_ac(x, outs), y, A, "fp32 resize") <= E.TAU
    dy = torch.randn(1, 1, *outs, generator=g)
    dx, dA = E.resize_bwd64(dy, ins)
    mats = [E.axis_weights(i, o)[0] for i, o in zip(ins, outs)]
    Mw = mats[2].clone()
    o = 100
    i = int(torch.nonzero(Mw[o]).max())
    assert float(Mw[o, i]) > 0.05
    Mw[o, i] = 0
    bad = E._apply(dy.double(), [mats[0].t(), mats[1].t(), Mw.t()])
    with pytest.raises(AssertionError, match=r"at \(n=0, c=0, t=\d+, h=\d+, w=%d\)" % i):
        R.check(bad, dx, dA, "one output missing from the gather")
