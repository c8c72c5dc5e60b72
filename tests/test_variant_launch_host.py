"""Host checks (no GPU) behind tests/test_variant_launches.py: every float64 reference of tests/variant_ref.py against torch
autograd in float64 of the reference project's own formulas, written out here (networks_3d.py:38-45: reparameterize_bern;
:110-138: Encode3DVAE_nb's gate and AdaptiveAvgPool3d(1); :456: code x map; losses.py:12-14: kl_bern_criterion); the same
operations in plain fp32 torch pass conv_ref.check at TAU with the derived error scales - the edges of the Bernoulli formulas
included -, and one seeded defect per operation fails it."""
import math

import pytest
import torch

import variant_ref as V

SHAPES = [(2, 8, 768), (2, 8, 192), (3, 5, 1), (2, 3, 257)]      # the fixture's coarsest levels (3-D, 2-D), S = 1, S = 257


def _inputs(B, C, S, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + 100 * B + 10 * C + S)
    r = lambda *sh: torch.randn(*sh, generator=g)
    return dict(f=r(B, C, S), logit=3 * r(B, S), dout=r(B, C, S), dbern=r(B, S), code=r(B, C), zmap=r(B, S), dz=r(B, C, S),
                gpool=r(B, C))


def _exact(got, ref, what):
    """Two float64 computations of one formula: equal to 1e-12 of the largest value."""
    assert got.shape == ref.shape, what
    assert float((got - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max())), what


# ------------------------------------------------------------------------------------------------ references vs autograd
@pytest.mark.parametrize("B,C,S", SHAPES)
def test_gate_reference_is_autograd_of_the_reference_formula(B, C, S):
    L = _inputs(B, C, S)
    f = L["f"].double().requires_grad_(True)
    logit = L["logit"].double().requires_grad_(True)
    bern = torch.sigmoid(logit)                       # networks_3d.py:133
    feats = bern[:, None, :] * f                      # :134
    ref = V.gate_fwd64(L["f"], L["logit"])
    _exact(ref["out"][0], feats.detach(), "gate out")
    _exact(ref["bern"][0], bern.detach(), "gate bern")
    for dout, ext in ((L["dout"], None), (None, L["dbern"]), (L["dout"], L["dbern"])):
        outs, gs = [], []
        if dout is not None:
            outs.append(feats)
            gs.append(dout.double())
        if ext is not None:
            outs.append(bern)
            gs.append(ext.double())
        df, dlogit = torch.autograd.grad(outs, [f, logit], gs, retain_graph=True, allow_unused=True)
        got = V.gate_bwd64(dout, L["f"], bern.detach(), ext)
        _exact(got["dlogit"][0], dlogit, "gate dlogit")
        _exact(got["df"][0], df if df is not None else torch.zeros_like(f), "gate df")


@pytest.mark.parametrize("B,C,S", SHAPES)
def test_pool_and_code_times_map_references_are_autograd(B, C, S):
    L = _inputs(B, C, S, 1)
    x = L["f"].double().requires_grad_(True)
    pooled = torch.nn.AdaptiveAvgPool1d(1)(x)[:, :, 0]            # AdaptiveAvgPool3d(1) on the flattened volume (:123)
    _exact(V.pool_fwd64(L["f"])[0], pooled.detach(), "pool")
    (dx,) = torch.autograd.grad(pooled, [x], L["gpool"].double())
    _exact(V.pool_bwd64(L["gpool"], S)[0], dx, "pool backward")
    code = L["code"].double().requires_grad_(True)
    zmap = L["zmap"].double().requires_grad_(True)
    z = code[:, :, None] * zmap[:, None, :]                      # z_vae_norm * z_vae_bern (:456)
    _exact(V.outer64(L["code"], L["zmap"], 1.0, S)[0], z.detach(), "code x map")
    dcode, dmap = torch.autograd.grad(z, [code, zmap], L["dz"].double())
    _exact(V.rowsum64(L["dz"], L["zmap"], 1.0)[0], dcode, "dcode")
    _exact(V.colsum64(L["dz"], L["code"])[0], dmap, "dmap")


def _kl_bern_criterion(x):                                        # losses.py:12-14
    KLD = torch.mul(x, torch.log(x + 1e-20) - math.log(0.5)) + torch.mul(1 - x, torch.log(1 - x + 1e-20) - math.log(1 - 0.5))
    return KLD.mean()


def _reparameterize_bern(x, eps):                                 # networks_3d.py:41 with its uniform draw handed in
    return torch.log(x + 1e-20) - torch.log(-torch.log(eps + 1e-20) + 1e-20)


def test_bernoulli_references_are_autograd_at_the_edges_too():
    """The references use the fp32 values of 1e-20 and log 0.5, the formulas above the float64 ones: they agree to TAU * A (the
    check the kernels take), with A from the derivation - 3e-8 relative in the constants is far inside it."""
    g = torch.Generator().manual_seed(5)
    x32, eps32 = V.edge_inputs(1500, g)
    dz = torch.randn(1500, generator=g)
    x = x32.double().requires_grad_(True)
    z = _reparameterize_bern(x, eps32.double())
    ref, A = V.reparam_bern_fwd64(x32, eps32)
    assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(z).all())
    V.check(z.detach(), ref, A, "reparam_bern vs the reference formula")
    (dx,) = torch.autograd.grad(z, [x], dz.double())
    ref, A = V.reparam_bern_bwd64(dz, x32)
    assert bool(torch.isfinite(ref).all())
    V.check(dx, ref, A, "reparam_bern backward vs autograd")
    x = x32.double().requires_grad_(True)
    kl = _kl_bern_criterion(x)
    ref, A = V.kl_bern_fwd64(x32)
    assert bool(torch.isfinite(ref))
    V.check(kl.detach().reshape(1), ref.reshape(1), A.reshape(1), "kl_bern vs the reference formula")
    (dx,) = torch.autograd.grad(kl, [x], torch.tensor(0.83, dtype=torch.float64))
    ref, A = V.kl_bern_bwd64(0.83, x32)
    assert bool(torch.isfinite(ref).all())
    # autograd's d/dx of x log(x + c) at x = 0 is log(c) + 0/(0 + c): the same closed form
    V.check(dx, ref, A, "kl_bern backward vs autograd")


# ------------------------------------------------------------------------------------------------ fp32 stand-ins and defects
def _sig32(l):
    return 1.0 / (1.0 + torch.exp(-l))


@pytest.mark.parametrize("B,C,S", SHAPES)
def test_plain_fp32_passes_at_tau_and_every_seeded_defect_fails(B, C, S):
    L = _inputs(B, C, S, 2)
    f, logit, dout, ext = L["f"], L["logit"], L["dout"], L["dbern"]
    g32 = _sig32(logit)
    ref = V.gate_fwd64(f, logit)
    V.check(g32, *ref["bern"], "fp32 bern")
    V.check(g32[:, None, :] * f, *ref["out"], "fp32 gate out")
    bref = V.gate_bwd64(dout, f, g32, ext)
    acc = (dout * f).sum(1) + ext
    V.check(acc * g32 * (1 - g32), *bref["dlogit"], "fp32 dlogit")
    V.check(dout * g32[:, None, :], *bref["df"], "fp32 df")
    if C > 1:
        with pytest.raises(AssertionError, match="tau"):          # a dropped channel in the gate sum
            V.check(V.gate_bwd64(dout, f, g32, ext, drop_channel=C - 1)["dlogit"][0].float(), *bref["dlogit"], "dropped channel")
    with pytest.raises(AssertionError, match="tau"):              # a missing (1 - g) factor
        V.check(V.gate_bwd64(dout, f, g32, ext, keep_factor=False)["dlogit"][0].float(), *bref["dlogit"], "missing 1 - g")
    pref = V.pool_fwd64(f)
    V.check(f.double().sum(2).float() * (1.0 / S), *pref, "fp32 pool")
    if S > 1:
        with pytest.raises(AssertionError, match="tau"):          # 1/S omitted from the pool
            V.check(V.pool_fwd64(f, with_scale=False)[0].float(), *pref, "pool without 1/S")
    V.check(L["gpool"][:, :, None].expand(B, C, S) * torch.tensor(1.0 / S), *V.pool_bwd64(L["gpool"], S), "fp32 pool backward")
    V.check(L["code"][:, :, None] * L["zmap"][:, None, :], *V.outer64(L["code"], L["zmap"], 1.0, S), "fp32 code x map")
    V.check((L["dz"] * L["zmap"][:, None, :]).double().sum(2).float(), *V.rowsum64(L["dz"], L["zmap"], 1.0), "fp32 dcode")
    V.check((L["dz"] * L["code"][:, :, None]).sum(1), *V.colsum64(L["dz"], L["code"]), "fp32 dmap")


def test_bernoulli_fp32_passes_at_the_edges_and_the_swapped_kl_term_fails():
    g = torch.Generator().manual_seed(6)
    x, eps = V.edge_inputs(1500, g)
    dz = torch.randn(1500, generator=g)
    c = torch.tensor(1e-20)
    l5 = torch.tensor(-0.6931471805599453)
    z = torch.log(x + c) - torch.log(-torch.log(eps + c) + c)
    assert bool(torch.isfinite(z).all())
    V.check(z, *V.reparam_bern_fwd64(x, eps), "fp32 reparam_bern")
    V.check(dz / (x + c), *V.reparam_bern_bwd64(dz, x), "fp32 reparam_bern backward")
    terms = x * (torch.log(x + c) - l5) + (1 - x) * (torch.log(1 - x + c) - l5)
    ref, A = V.kl_bern_fwd64(x)
    V.check(terms.double().mean().float().reshape(1), ref.reshape(1), A.reshape(1), "fp32 kl_bern")
    k = torch.tensor(0.83) / 1500.0
    dx = k * (torch.log(x + c) + x / (x + c) - torch.log(1 - x + c) - (1 - x) / (1 - x + c))
    assert bool(torch.isfinite(dx).all())
    V.check(dx, *V.kl_bern_bwd64(0.83, x), "fp32 kl_bern backward")
    with pytest.raises(AssertionError, match="tau"):              # the swapped KL term: x in place of 1 - x
        V.check(V.kl_bern_fwd64(x, swapped=True)[0].float().reshape(1), ref.reshape(1), A.reshape(1), "swapped KL term")
    # without the edges too: the defect is not an edge effect
    xi = torch.rand(1500, generator=g) * 0.98 + 0.01
    ref, A = V.kl_bern_fwd64(xi)
    with pytest.raises(AssertionError, match="tau"):
        V.check(V.kl_bern_fwd64(xi, swapped=True)[0].float().reshape(1), ref.reshape(1), A.reshape(1), "swapped KL term")
