"""tests/param_ref.py against what it stands for, on the CPU: the float64 references against torch.nn.utils.spectral_norm,
torch.optim.Adam and torch.nn.utils.clip_grad_norm_ in double (1e-12 of A); the power of conv_ref.check with param_ref's
error scales (fp32 simulations of the kernels' arithmetic pass at TAU with room, each seeded defect is rejected); and the
launch lists of param_ref against the modules."""
import pytest
import torch
import torch.nn as nn

import conv_ref as R
import param_ref as P

TIGHT = 1e-12
REJECT = r"\|got - ref\| / A"


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------ launch lists
def test_launch_lists():
    """The six (Co, K) a critic hands to one SpectralNormWeightBatch launch (3-D and 2-D, nfc = 64) and the arena sizes and
    Adam ranges of the video config are what param_ref lists."""
    import bench
    from hp_vae_gan_amd import optim, train
    from hp_vae_gan_amd.modules import networks_2d
    opt, netG, netD = P.video_nets(1)
    assert int(opt.nfc) == 64
    assert P.sn_layers_of(netD) == P.SN_LAYERS_3D
    assert P.sn_layers_of(networks_2d.WDiscriminator2D(bench.image_opt("cpu"))) == P.SN_LAYERS_2D
    for tail, full in ((P.SN_TAIL_3D, P.SN_LAYERS_3D), (P.SN_TAIL_2D, P.SN_LAYERS_2D)):
        assert tail[:5] == full[:5] and tail[5] == (1, full[5][1])
    assert optim.ParamArena(netD).total == P.ARENA_FLOATS["D"]
    for stage in (1, 9):
        opt, netG, _ = P.video_nets(stage)
        arena = optim.ParamArena(netG)
        assert arena.total == P.ARENA_FLOATS["G%d" % stage]
        adam = optim.FlatAdam(arena, train.generator_param_groups(opt, netG), betas=(opt.beta1, 0.999))
        want = P.ADAM_RANGES["G%d" % stage]
        assert [(g["lo"], g["hi"]) for g in adam.groups] == [(lo, hi) for lo, hi, _ in want]
        for g, (_, _, lr) in zip(adam.groups, want):
            assert g["lr"] == pytest.approx(lr, rel=1e-12)
        assert all(g["m"].numel() == g["hi"] - g["lo"] for g in adam.groups)
    assert len({lr for _, _, lr in P.ADAM_RANGES["G1"]}) == 2


# ------------------------------------------------------------------------------------------------ references vs torch
@pytest.mark.parametrize("dims,cin,cout", [(3, 3, 8), (3, 8, 1), (2, 5, 7)], ids=["3d-3to8", "3d-8to1", "2d-5to7"])
def test_sn_reference_against_torch_spectral_norm(dims, cin, cout):
    """param_ref's v, u, sigma, w_eff and dW_orig against nn.utils.spectral_norm on a double Conv3d / Conv2d (one power
    iteration, eps 1e-12, autograd through weight_orig), training and eval mode."""
    torch.manual_seed(7 + dims + cout)
    conv = (nn.Conv3d if dims == 3 else nn.Conv2d)(cin, cout, 3, padding=1).double()
    conv = nn.utils.spectral_norm(conv, n_power_iterations=1, eps=1e-12)
    W = conv.weight_orig.detach().clone()
    u0 = conv.weight_u.clone()
    x = torch.randn(1, cin, *((4,) * dims), dtype=torch.float64)
    dW = torch.randn(W.shape, dtype=torch.float64, generator=_gen(3))
    for training in (True, False):
        conv.train(training)
        u_in, v_in = conv.weight_u.clone(), conv.weight_v.clone()
        conv.weight_orig.grad = None
        conv(x)
        w_eff = conv.weight
        (w_eff * dW).sum().backward()
        if training:
            v, vA = P.sn_v64(W, u_in)
            u, uA = P.sn_u64(W, v)
            R.check(conv.weight_v, v, vA, "v", tau=TIGHT)
            R.check(conv.weight_u, u, uA, "u", tau=TIGHT)
        else:
            assert torch.equal(conv.weight_u, u_in) and torch.equal(conv.weight_v, v_in)
            u, v = u_in, v_in
        (sig, sigA), (inv, invA) = P.sn_sigma64(W, u, v)
        assert float(sigA) >= abs(float(sig)) > 0
        got_sig = (W.reshape(-1)[W.abs().argmax()] / w_eff.detach().reshape(-1)[W.abs().argmax()]).reshape(1)
        R.check(got_sig, sig.reshape(1), sigA.reshape(1), "sigma", tau=1e-10)   # (recovered through a quotient)
        R.check(1 / got_sig, inv.reshape(1), invA.reshape(1), "1/sigma", tau=1e-10)
        ref, A = P.sn_weff64(W, sig)
        R.check(w_eff.detach(), ref, A, "w_eff", tau=TIGHT, names=R.WEIGHT_NAMES[dims + 2])
        ref, A = P.sn_bwd64(dW, W, sig, u, v)
        R.check(conv.weight_orig.grad, ref, A, "dW_orig", tau=TIGHT, names=R.WEIGHT_NAMES[dims + 2])
        pre = torch.randn(W.shape, dtype=torch.float64, generator=_gen(4))
        ref2, A2 = P.sn_bwd64(dW, W, sig, u, v, preset=pre)
        assert torch.allclose(ref2, ref + pre, rtol=0, atol=1e-14) and bool((A2 >= A).all())
    assert cout == 1 or not torch.equal(conv.weight_u, u0)


def test_adam_reference_against_torch_adam():
    """Five steps of param_ref.adam_step64 against torch.optim.Adam in double with the fp32 hyperparameters."""
    g0 = _gen(5)
    n = 257
    lr, b1, b2, eps = P._f32(5e-4), P._f32(0.5), P._f32(0.999), P._f32(1e-8)
    assert b2 != 0.999 and abs(b2 - 0.999) < 2e-8
    p = nn.Parameter(torch.randn(n, dtype=torch.float64, generator=g0))
    opt = torch.optim.Adam([p], lr=lr, betas=(b1, b2), eps=eps)
    m, v = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    pr = p.detach().clone()
    for t in range(1, 6):
        g = torch.randn(n, dtype=torch.float64, generator=g0) * 10.0 ** float(torch.randint(-3, 2, (1,), generator=g0))
        p.grad = g.clone()
        before = pr.clone()
        opt.step()
        (_, mA), (_, vA) = P.adam_moments64(g, m, v, b1, b2)
        pr, m, v = P.adam_step64(pr, g, m, v, t, lr, b1, b2, eps)
        st = opt.state[p]
        R.check(st["exp_avg"], m, mA, "step %d m" % t, tau=TIGHT)
        R.check(st["exp_avg_sq"], v, vA, "step %d v" % t, tau=TIGHT)
        R.check(before - p.detach(), before - pr, (before - pr).abs() + 1e-3 * before.abs(), "step %d update" % t, tau=TIGHT)


@pytest.mark.parametrize("scale", [10.0, 1e-3, 0.0], ids=["clipped", "below", "zero"])
def test_clip_reference_against_torch_clip(scale):
    ps = [nn.Parameter(torch.zeros(s, dtype=torch.float64)) for s in (33, 1000)]
    for i, q in enumerate(ps):
        q.grad = scale * torch.randn(q.shape, dtype=torch.float64, generator=_gen(20 + i))
    g = torch.cat([q.grad.reshape(-1) for q in ps]).clone()
    total_t = nn.utils.clip_grad_norm_(ps, 5.0)
    (total, tA), (coef, cA) = P.clip64((g * g).sum(), 5.0)
    assert float(tA) == float(total) and float(cA) == float(coef)
    assert abs(float(total_t) - float(total)) <= TIGHT * float(total)
    assert (float(coef) < 1) == (scale == 10.0)
    ref, A = P.clip_apply64(g, coef)
    R.check(torch.cat([q.grad.reshape(-1) for q in ps]), ref, A, "clipped gradient", tau=TIGHT)
    if scale != 10.0:
        assert float(coef) == 1.0 and torch.equal(ref, g)


# ------------------------------------------------------------------------------------------------ checker power
def _fp32_sn_fwd(W, u_in, eps=P.SN_EPS, drop_slice=None, stale_u=False):
    """The power iteration in fp32 (norms in double, as the kernel): (v, u', sigma).  drop_slice = (S, s): the rows
    o % S == s are missing from W^T u (one of the S row slices that meet in LDS); stale_u: sigma from u_in."""
    M = W.reshape(W.shape[0], -1).float()
    keep = torch.ones(M.shape[0])
    if drop_slice is not None:
        S, s = drop_slice
        keep[s::S] = 0
    t = (M * keep[:, None]).t() @ u_in.float()
    v = (t / max(float(t.double().norm()), eps)).float()
    s_ = M @ v
    u = (s_ / max(float(s_.double().norm()), eps)).float()
    sigma = ((u_in.float() if stale_u else u).double() @ s_.double()).float()
    return v, u, sigma


def _fp32_sn_bwd(dW, W, sigma, u, v, first_chunk_only=False, row_shift=False):
    """The backward in fp32 (dot in double).  first_chunk_only: coef from the first SN_CHUNK elements' partial alone;
    row_shift: u[o + 1] for the elements after the first chunk boundary."""
    Co = W.shape[0]
    d, M = dW.reshape(Co, -1).float(), W.reshape(Co, -1).float()
    K = d.shape[1]
    prod = (d.double() * M.double()).reshape(-1)
    dot = prod[:P.SN_CHUNK].sum() if first_chunk_only else prod.sum()
    sg = sigma.float().reshape(())
    coef = (dot / (sg.double() * sg.double())).float()
    j = torch.arange(Co * K)
    o = j // K
    if row_shift:
        o = torch.where(j >= P.SN_CHUNK, (o + 1).clamp(max=Co - 1), o)
    return (d.reshape(-1) / sg - coef * u.float()[o] * v.float()[j % K]).reshape(dW.shape)


def _sn_data(Co, K, seed):
    g = _gen(seed)
    W = torch.randn(Co, K, generator=g) / K ** 0.5
    u = torch.nn.functional.normalize(torch.randn(Co, generator=g), dim=0)
    return W, u, torch.randn(Co, K, generator=g)


@pytest.mark.parametrize("Co,K,S", [(64, 1728, 2), (64, 68, 8), (64, 81, 4)], ids=["64x1728", "64x68", "64x81"])
def test_checker_power_spectral_norm(Co, K, S):
    W, u_in, dW = _sn_data(Co, K, 31 + K)
    v, u, sigma = _fp32_sn_fwd(W, u_in)
    vr, vA = P.sn_v64(W, u_in)
    ur, uA = P.sn_u64(W, v)
    (sr, sA), (ir, iA) = P.sn_sigma64(W, u, v)
    ratios = {"v": R.check(v, vr, vA, "fp32 v"), "u": R.check(u, ur, uA, "fp32 u"),
              "sigma": R.check(sigma.reshape(1), sr.reshape(1), sA.reshape(1), "fp32 sigma"),
              "1/sigma": R.check((1 / sigma.double()).float().reshape(1), ir.reshape(1), iA.reshape(1), "fp32 1/sigma")}
    wr, wA = P.sn_weff64(W, sigma)
    ratios["w_eff"] = R.check(W / sigma, wr, wA, "fp32 w_eff", tau=P.U1)
    with pytest.raises(AssertionError, match=REJECT):
        R.check(W / (sigma * (1 + 2.0 ** -22)), wr, wA, "w_eff divided by a sigma two ulps off", tau=P.U1)
    # one of the S row slices left out of W^T u
    v_bad, _, _ = _fp32_sn_fwd(W, u_in, drop_slice=(S, S - 1))
    with pytest.raises(AssertionError, match=REJECT):
        R.check(v_bad, vr, vA, "row slice dropped")
    # sigma with the u from before the iteration
    _, _, sig_bad = _fp32_sn_fwd(W, u_in, stale_u=True)
    with pytest.raises(AssertionError, match=REJECT):
        R.check(sig_bad.reshape(1), sr.reshape(1), sA.reshape(1), "sigma from the stale u")
    # backward
    br, bA = P.sn_bwd64(dW, W, sigma, u, v)
    ratios["bwd"] = R.check(_fp32_sn_bwd(dW, W, sigma, u, v), br, bA, "fp32 backward")
    with pytest.raises(AssertionError, match=REJECT):
        R.check(_fp32_sn_bwd(dW, W, sigma, u, v, first_chunk_only=True), br, bA, "coef from the first chunk only")
    assert Co * K > P.SN_CHUNK
    with pytest.raises(AssertionError, match=REJECT):
        R.check(_fp32_sn_bwd(dW, W, sigma, u, v, row_shift=True), br, bA, "u[o] one row off after the chunk boundary")
    print("\nfp32 simulation (%d, %d), worst |got - ref| / A (tau %.0e): %s" % (
        Co, K, P.TAU, ", ".join("%s %.2e" % kv for kv in ratios.items())))
    assert max(v for k, v in ratios.items() if k != "w_eff") <= P.TAU / 10      # room: a tenth of TAU
    assert ratios["w_eff"] <= P.U


def _fp32_adam(p, g, m, v, t, lr, b1, b2, eps, t_bias=None, no_factor=False, beta2_double=False):
    """adam_kernel's arithmetic in fp32 -> (p', m', v').  t_bias: the count the bias corrections use; no_factor: v' without
    (1 - beta2); beta2_double: v' and its bias correction with the double 0.999 instead of fl32(0.999)."""
    f = torch.float32
    tb = float(t if t_bias is None else t_bias)
    lr, b1, b2, eps = (torch.tensor(x, dtype=f) for x in (lr, b1, b2, eps))
    one = torch.tensor(1.0, dtype=f)
    bc1 = one - b1.pow(tb)
    mi = b1 * m + (one - b1) * g
    if beta2_double:
        vi = (0.999 * v.double() + (1 - 0.999) * g.double() * g.double()).float()
        bc2s = torch.tensor((1 - 0.999 ** tb) ** 0.5, dtype=f)
    else:
        vi = b2 * v + (g * g if no_factor else (one - b2) * g * g)
        bc2s = (one - b2.pow(tb)).sqrt()
    return p - (lr / bc1) * (mi / (vi.sqrt() / bc2s + eps)), mi, vi


def _adam_data(n, seed, zero_moments=False):
    g0 = _gen(seed)
    p = torch.randn(n, generator=g0)
    p[: n // 4] = 0                                   # the update judged alone
    g = torch.randn(n, generator=g0) * 10.0 ** torch.randint(-4, 1, (n,), generator=g0).float()
    m = 0.1 * torch.randn(n, generator=g0)
    v = (0.1 * torch.randn(n, generator=g0)) ** 2
    if zero_moments:
        m, v = torch.zeros(n), torch.zeros(n)
    return p, g, m, v


def _adam_check(out, p, g, m, v, t, hp, what):
    """conv_ref.check of (p', m', v') against param_ref -> the worst ratios of m', v', the update, and the update where
    p = 0 (there no rounding of p' stands beside it: the other elements' ratio reaches TAU whenever fl(p - upd) rounds by
    its full u |p|, which is a bound and not a tolerance)."""
    lr, b1, b2, eps = hp
    p1, m1, v1 = out
    (mr, mA), (vr, vA) = P.adam_moments64(g, m, v, b1, b2)
    rm = R.check(m1, mr, mA, what + ": m")
    rv = R.check(v1, vr, vA, what + ": v")
    ur, uA = P.adam_update64(p, m1, v1, t, lr, b1, b2, eps)
    ru = R.check(p.double() - p1.double(), ur, uA, what + ": update")
    z = p == 0
    rz = R.check(-p1.double()[z], ur[z], uA[z], what + ": update at p = 0")
    return rm, rv, ru, rz


@pytest.mark.parametrize("beta1", [0.5, 0.9])
def test_checker_power_adam(beta1):
    hp = (5e-4, beta1, 0.999, 1e-8)
    worst = 0.0
    for t in (1, 2, 3, 10, 1000, 100000):
        p, g, m, v = _adam_data(4099, 40 + t % 7)
        r = _adam_check(_fp32_adam(p, g, m, v, t, *hp), p, g, m, v, t, hp, "fp32 Adam t=%d" % t)
        worst = max(worst, r[0], r[1], r[3] / 5)
        print("fp32 Adam beta1 %.1f t=%-6d worst |got - ref| / A: m %.2e v %.2e update %.2e, at p = 0 %.2e" % ((beta1, t) + r))
    assert worst <= P.TAU / 10                        # room: a tenth of TAU for the moments, half for the update at p = 0
    # bias corrections with t - 1
    for t in (2, 10, 1000):
        p, g, m, v = _adam_data(4099, 50 + t % 7)
        with pytest.raises(AssertionError, match=r": update: " + REJECT):
            _adam_check(_fp32_adam(p, g, m, v, t, *hp, t_bias=t - 1), p, g, m, v, t, hp, "bias correction with t - 1")
    # second moment without its (1 - beta2) factor
    p, g, m, v = _adam_data(4099, 61)
    with pytest.raises(AssertionError, match=r": v: " + REJECT):
        _adam_check(_fp32_adam(p, g, m, v, 3, *hp, no_factor=True), p, g, m, v, 3, hp, "no (1 - beta2)")
    # 1 - 0.999 in double instead of 1 - fl32(0.999): 1.29e-5 of (1 - beta2) g^2, seen in v' from zero moments (the first
    # step); the update's own bound at t = 1 (TAU + c(beta2, 1) / 2 = 7e-5) does not see the 6.4e-6 it moves the update by
    p, g, m, v = _adam_data(4099, 62, zero_moments=True)
    with pytest.raises(AssertionError, match=r": v: " + REJECT):
        _adam_check(_fp32_adam(p, g, m, v, 1, *hp, beta2_double=True), p, g, m, v, 1, hp, "1 - 0.999 in double")
    r = _adam_check(_fp32_adam(p, g, m, v, 1, *hp), p, g, m, v, 1, hp, "fp32 Adam from zero moments")
    assert max(r[0], r[1], r[3] / 5) <= P.TAU / 10


def test_adam_update_scale_sees_what_p_hides():
    """A 2 % error of the update passes 1e-5 of |p| (the measure of the older test) and fails the update's own scale."""
    hp = (5e-4, 0.5, 0.999, 1e-8)
    p, g, m, v = _adam_data(4099, 70, zero_moments=True)      # the first step: |upd| = lr
    p1, m1, v1 = _fp32_adam(p, g, m, v, 1, *hp)
    bad = p - 1.02 * (p - p1)
    assert float((bad - p1).abs().max()) <= 1.1e-5 * float(p.abs().max())
    with pytest.raises(AssertionError, match=r": update: " + REJECT):
        _adam_check((bad, m1, v1), p, g, m, v, 1, hp, "update 2 % too large")


def test_bias_conditioning_values():
    """c(beta, t) = u (1 + beta^t) / (1 - beta^t): 2000 u at (0.999, 1), 3 u at (0.5, 1), u once beta^t has died out."""
    assert P.bias_conditioning(0.999, 1) == pytest.approx(P.U * 1.999 / (1 - P._f32(0.999)), rel=1e-6)
    assert P.bias_conditioning(0.999, 1) > P.TAU
    assert P.bias_conditioning(0.5, 1) == pytest.approx(3 * P.U)
    assert P.bias_conditioning(0.999, 100000) == pytest.approx(P.U)
