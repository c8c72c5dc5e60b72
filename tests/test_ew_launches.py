"""Every BatchNorm, resize, gradient-penalty and loss launch the benchmark's pyramids make (tests/ew_ref.py: the level shapes of
conv_ref.level_shapes - video, video8, image), at its real size, with the library's own size rules, element by element
against float64: |got - ref| <= tau * A per element, A = the error scale of tests/ew_ref.py.

BatchNorm (C = 64, every level shape): B = 2 and B = 1 with groups = 1, B = 4 with groups = 2 (the merged rec + rand
generator pass); the launch plan (fused or three launches per group, nsplit, vector width) of ew_ref.BN_PLANS; forward
output, the per-group statistics and the running buffers (updated once per group, rec first); backward dr, dgamma, dbeta
in the fresh and the direct-slot (.grad preset, accumulate) form.  LeakyReLU is off for B = 1 (fused path) and for the
three-launch B = 2 launch of the finest level.  The batch-split BatchNorm (BNActSync, two ranks of B = 1, all-reduce by
hand) at one level per vector width and at the finest level; the second-order BatchNorm (BNActBwd's backward) at the
baselines critic's padded video8 volumes, B = 2.

Resize: the generator's level i -> i + 1 resizes of its 3-channel images (modules/_nets.py; utils/images.interpolate and
upscale are not called by the train step or train.py, and the data front end resizes with frames.hip), at B = 4: plain,
with a noise tensor, with the in-kernel noise of UpsampleACNoise (rows below first_noisy = 2 get none; the noise is
hpvg_normal_f32's stream at the same seed, call and iteration), backward with dy alone and with dy + dy2.
Gradient penalty on (2, 3, level) gradients, MSE on (2, 3, level), the critic terms (mean-scaled) on (2, 1, level), sqsum
on a level's 64-channel activation, KL at the latent shape (2, 128, level 0) of each pyramid.

Every launch that takes a workspace runs a second time with every workspace byte set to 0xFF and must reproduce the first
result bit for bit.  The float64 references run through torch's own ops on the GPU; the inputs of a level are shared by
its batch sizes (B < 4: the first B samples) and freed when the next level starts."""
import ctypes
import zlib

import pytest
import torch

import conv_ref as R
import ew_ref as E

pytestmark = pytest.mark.gpu

DEV = "cuda"
_STATS = {}
_LEVEL = {}


@pytest.fixture(scope="module")
def ops():
    import hp_vae_gan_amd  # noqa: F401
    from hp_vae_gan_amd import ops as _ops
    yield _ops
    _LEVEL.clear()
    if _STATS:
        print("\nworst |got - ref| / A per (op, path, V) (tau %.0e, statistics %.0e):" % (E.TAU, E.TAU_STAT))
        for (q, k), v in sorted(_STATS.items()):
            print("  %-22s %-14s %.3e" % (q, k, v))


@pytest.fixture(scope="module")
def lib(ops):
    from hp_vae_gan_amd import lib as hplib
    return hplib.load()


def _check(got, ref, A, what, quantity, key, tau=E.TAU):
    r = R.check(got, ref, A, what, tau=tau)
    k = (quantity, key)
    _STATS[k] = max(_STATS.get(k, 0.0), r)


def _check_scalar(got, ref, A, what, quantity, key):
    _check(got.reshape(1), ref.reshape(1), A.reshape(1).float(), what, quantity, key)


def _fill_ws(ops):
    for buf in ops._ws_cache.values():
        buf.fill_(0xFF)


def _same(r1, r2, tag):
    for k, v in r1.items():
        assert torch.equal(r2[k], v), tag + "%s differs after the workspace was filled with 0xFF" % k


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _level(sp):
    """Inputs of one level shape, shared by its batch sizes: r with per-channel offsets and spreads, dh, G, BatchNorm
    parameters and running buffers (C = 64, 4 samples)."""
    key = tuple(sp)
    if _LEVEL.get("key") == key:
        return _LEVEL
    _LEVEL.clear()
    torch.cuda.empty_cache()
    g = _gen(zlib.crc32(repr(key).encode()))
    C, nd = E.BN_C, len(sp)
    one = (1, C) + (1,) * nd
    r = torch.randn(4, C, *sp, generator=g, device=DEV) * (0.5 + torch.rand(one, generator=g, device=DEV)) \
        + (torch.rand(one, generator=g, device=DEV) * 2 - 1)
    _LEVEL.update(key=key, r=r, dh=torch.randn(4, C, *sp, generator=g, device=DEV),
                  gamma=1 + 0.3 * torch.randn(C, generator=g, device=DEV), beta=0.3 * torch.randn(C, generator=g, device=DEV),
                  rm=0.1 * torch.randn(C, generator=g, device=DEV), rv=1 + 0.2 * torch.rand(C, generator=g, device=DEV),
                  base_g=torch.randn(C, generator=g, device=DEV), base_b=torch.randn(C, generator=g, device=DEV))
    return _LEVEL


def _pathkey(plan):
    fused, _, V = plan
    return "%s V=%d" % ("fused" if fused else "3-launch", V)


# ------------------------------------------------------------------------------------------------ BatchNorm
BN_CASES = E.bn_launches()


def _bn_id(c):
    cfg, lvl, sp, B, groups = c
    return "%s-s%d-B%d-g%d" % (cfg, lvl, B, groups)


@pytest.mark.parametrize("cfg,lvl,sp,B,groups", BN_CASES, ids=[_bn_id(c) for c in BN_CASES])
def test_bn_launch_against_float64(ops, lib, cfg, lvl, sp, B, groups):
    S = E.spatial(sp)
    plan = E.bn_plan_of(lib, B, S, groups)
    tag = "%s level %d %s B=%d groups=%d: " % (cfg, lvl, tuple(sp), B, groups)
    assert plan == E.expected_plan(sp, B, groups), tag + "plan (fused, nsplit, V) %s" % (plan,)
    lrelu = not (B == 1 or (B == 2 and not plan[0]))
    L = _level(sp)
    r, dh = L["r"][:B], L["dh"][:B]
    pk = _pathkey(plan) + (" g2" if groups == 2 else "")

    def launch():
        out = {}
        rm, rv = L["rm"].clone(), L["rv"].clone()
        rl = r.clone().requires_grad_(True)
        gl, bl = L["gamma"].clone().requires_grad_(True), L["beta"].clone().requires_grad_(True)
        h = ops.BNAct.apply(rl, gl, bl, rm, rv, E.BN_MOMENTUM, E.BN_EPS, lrelu, groups)
        out["stats"] = h.grad_fn.saved_tensors[1].clone()
        out["dr"], out["dg"], out["db"] = torch.autograd.grad(h, [rl, gl, bl], dh, retain_graph=True)
        gl.grad, bl.grad = L["base_g"].clone(), L["base_b"].clone()
        h.backward(dh)
        out.update(h=h.detach(), rm=rm, rv=rv, dr_slot=rl.grad, dg_slot=gl.grad, db_slot=bl.grad)
        torch.cuda.synchronize()
        return out

    o = launch()
    ref = E.bn_fwd64(r, L["gamma"], L["beta"], L["rm"], L["rv"], groups=groups, lrelu=lrelu)
    _check(o["h"], *ref["h"], tag + "h", "bn.fwd" + (".lrelu" if lrelu else ""), pk)
    st = o["stats"]
    assert tuple(st.shape) == (groups, 4, E.BN_C)
    for j, name in enumerate(("mean", "invstd", "scale", "shift")):
        _check(st[:, j], *ref[name], tag + name, "bn.stat", pk, tau=E.TAU_STAT)
    _check(o["rm"], *ref["rm"], tag + "running_mean", "bn.running", pk, tau=E.TAU_STAT)
    _check(o["rv"], *ref["rv"], tag + "running_var", "bn.running", pk, tau=E.TAU_STAT)
    del ref
    bwd = E.bn_bwd64(dh, r, st, groups=groups, lrelu=lrelu, base_gamma=None, base_beta=None)
    _check(o["dr"], *bwd["dr"], tag + "dr", "bn.bwd" + (".lrelu" if lrelu else ""), pk)
    _check(o["dg"], *bwd["dgamma"], tag + "dgamma", "bn.dgamma", pk)
    _check(o["db"], *bwd["dbeta"], tag + "dbeta", "bn.dbeta", pk)
    del bwd
    assert torch.equal(o["dr_slot"], o["dr"]), tag + "dr of the direct-slot backward differs"
    slot = E.bn_bwd64(dh, r, st, groups=groups, lrelu=lrelu, base_gamma=L["base_g"], base_beta=L["base_b"])
    _check(o["dg_slot"], *slot["dgamma"], tag + "dgamma, direct slot", "bn.dgamma.slot", pk)
    _check(o["db_slot"], *slot["dbeta"], tag + "dbeta, direct slot", "bn.dbeta.slot", pk)
    del slot
    _fill_ws(ops)
    _same(o, launch(), tag)


# the batch-split BatchNorm: one level per vector width (4, 2, 1), and the finest level
SYNC_SHAPES = [(4, 18, 33), (5, 57, 102), (5, 45, 81), (13, 144, 256)]


@pytest.mark.parametrize("sp", SYNC_SHAPES, ids=["x".join(map(str, s)) for s in SYNC_SHAPES])
def test_bn_batch_split_against_float64(ops, lib, sp):
    """Two ranks of B = 1 with the per-channel sums added by hand (as the all-reduce would): h, statistics, running buffers
    and dr against the float64 BatchNorm of the whole B = 2 batch; the ranks' dgamma / dbeta shares add up to its
    parameter gradients."""
    S = E.spatial(sp)
    L = _level(sp)
    C = E.BN_C
    r, dh = L["r"][:2], L["dh"][:2]
    V = E.bn_plan_of(lib, 1, S, 1)[2]
    tag = "batch-split %s: " % (tuple(sp),)
    from hp_vae_gan_amd import lib as hplib
    fwd_local = {}
    for rank in (0, 1):
        x = r[rank:rank + 1]
        ws = ops.workspace(hplib.call("hpvg_bn_ws_bytes", C), x.device)
        sums = torch.empty(C, 2, dtype=torch.float64, device=DEV)
        hplib.call("hpvg_bn_sums_f32", hplib.ptr(x), hplib.ptr(sums), hplib.ptr(ws), ctypes.c_size_t(ws.numel()), 1, C,
                   ctypes.c_long(S), hplib.stream())
        fwd_local[rank] = sums

    def run(rank, partner_bwd):
        calls = []

        def allreduce(t):
            calls.append(t.clone())
            t.add_(fwd_local[1 - rank] if len(calls) == 1 else partner_bwd)

        gl, bl = L["gamma"].clone().requires_grad_(True), L["beta"].clone().requires_grad_(True)
        rl = r[rank:rank + 1].clone().requires_grad_(True)
        rm, rv = L["rm"].clone(), L["rv"].clone()
        h = ops.BNActSync.apply(rl, gl, bl, rm, rv, E.BN_MOMENTUM, E.BN_EPS, True, allreduce, 2)
        stats = h.grad_fn.saved_tensors[1].clone()
        grads = torch.autograd.grad(h, [rl, gl, bl], dh[rank:rank + 1])
        return dict(h=h.detach(), rm=rm, rv=rv, stats=stats, dr=grads[0], dg=grads[1], db=grads[2]), calls[1]

    bwd_local = {rank: run(rank, torch.zeros(C, 2, dtype=torch.float64, device=DEV))[1] for rank in (0, 1)}
    outs = {rank: run(rank, bwd_local[1 - rank])[0] for rank in (0, 1)}
    torch.cuda.synchronize()
    key = "V=%d" % V
    ref = E.bn_fwd64(r, L["gamma"], L["beta"], L["rm"], L["rv"], groups=1, lrelu=True)
    _check(torch.cat([outs[0]["h"], outs[1]["h"]]), *ref["h"], tag + "h", "sync.fwd.lrelu", key)
    for rank in (0, 1):
        for j, name in enumerate(("mean", "invstd", "scale", "shift")):
            _check(outs[rank]["stats"][j:j + 1], *ref[name], tag + "rank %d %s" % (rank, name), "sync.stat", key, tau=E.TAU_STAT)
        _check(outs[rank]["rm"], *ref["rm"], tag + "running_mean", "sync.running", key, tau=E.TAU_STAT)
        _check(outs[rank]["rv"], *ref["rv"], tag + "running_var", "sync.running", key, tau=E.TAU_STAT)
    assert torch.equal(outs[0]["stats"], outs[1]["stats"]), tag + "the ranks' statistics differ"
    del ref
    bwd = E.bn_bwd64(dh, r, outs[0]["stats"].view(1, 4, C), groups=1, lrelu=True)
    _check(torch.cat([outs[0]["dr"], outs[1]["dr"]]), *bwd["dr"], tag + "dr", "sync.bwd.lrelu", key)
    _check(outs[0]["dg"] + outs[1]["dg"], *bwd["dgamma"], tag + "dgamma (sum of the shares)", "sync.dgamma", key)
    _check(outs[0]["db"] + outs[1]["db"], *bwd["dbeta"], tag + "dbeta (sum of the shares)", "sync.dbeta", key)


PADDED = E.padded_shapes()


@pytest.mark.parametrize("sp", PADDED, ids=["x".join(map(str, s)) for s in PADDED])
def test_bn_second_order_against_float64(ops, lib, sp):
    """BNActBwd's backward (hpvg_bn_act_bwd2_f32) at the baselines critic's padded video8 volumes, B = 2: g_dh, g_r,
    g_gamma against the closed form in float64, given the statistics of a BNAct forward at the same shape."""
    S = E.spatial(sp)
    plan = E.bn_plan_of(lib, 2, S, 1)
    assert plan == E.BN2_PLANS[tuple(sp)]
    tag = "second order %s B=2: " % (tuple(sp),)
    g = _gen(zlib.crc32(repr(("bwd2",) + tuple(sp)).encode()))
    _LEVEL.clear()
    torch.cuda.empty_cache()
    C = E.BN_C
    one = (1, C, 1, 1, 1)
    r = torch.randn(2, C, *sp, generator=g, device=DEV) * (0.5 + torch.rand(one, generator=g, device=DEV)) \
        + (torch.rand(one, generator=g, device=DEV) * 2 - 1)
    dh = torch.randn(2, C, *sp, generator=g, device=DEV)
    G = torch.randn(2, C, *sp, generator=g, device=DEV)
    gamma, beta = 1 + 0.3 * torch.randn(C, generator=g, device=DEV), 0.3 * torch.randn(C, generator=g, device=DEV)
    rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    h = ops.BNAct.apply(r, gamma.clone().requires_grad_(True), beta, rm, rv, E.BN_MOMENTUM, E.BN_EPS, True, 1)
    stats = h.grad_fn.saved_tensors[1].clone()
    del h

    def launch():
        dhl, rl, gl = dh.clone().requires_grad_(True), r.clone().requires_grad_(True), gamma.clone().requires_grad_(True)
        dr, _, _ = ops.BNActBwd.apply(dhl, rl, gl, stats, True)
        g_dh, g_r, g_g = torch.autograd.grad(dr, [dhl, rl, gl], G)
        torch.cuda.synchronize()
        return {"dr": dr.detach(), "g_dh": g_dh, "g_r": g_r, "g_gamma": g_g}

    o = launch()
    pk = _pathkey(plan)
    ref = E.bn_bwd2_64(dh, G, r, stats, lrelu=True)
    _check(o["g_dh"], *ref["g_dh"], tag + "g_dh", "bn2.g_dh", pk)
    _check(o["g_r"], *ref["g_r"], tag + "g_r", "bn2.g_r", pk)
    _check(o["g_gamma"], *ref["g_gamma"], tag + "g_gamma", "bn2.g_gamma", pk)
    del ref
    first = E.bn_bwd64(dh, r, stats.view(1, 4, C), groups=1, lrelu=True)
    _check(o["dr"], *first["dr"], tag + "dr (first order)", "bn.bwd.lrelu", pk)
    del first
    _fill_ws(ops)
    _same(o, launch(), tag)


# ------------------------------------------------------------------------------------------------ resize
RESIZE_CASES = E.resize_launches()


@pytest.mark.parametrize("cfg,lvl,ins,outs", RESIZE_CASES, ids=["%s-s%d" % (c[0], c[1]) for c in RESIZE_CASES])
def test_resize_launch_against_float64(ops, lib, cfg, lvl, ins, outs):
    B, C, first_noisy, amp = 4, E.RESIZE_C, 2, 0.37
    tag = "%s resize %s -> %s: " % (cfg, tuple(ins), tuple(outs))
    g = _gen(zlib.crc32(repr((cfg, lvl)).encode()))
    x = torch.randn(B, C, *ins, generator=g, device=DEV)
    noise = torch.randn(B, C, *outs, generator=g, device=DEV)
    dy = torch.randn(B, C, *outs, generator=g, device=DEV)
    dy2 = torch.randn(B, C, *outs, generator=g, device=DEV)
    st = ops._rng(torch.device(DEV))
    call0 = 1000 + lvl
    from hp_vae_gan_amd import lib as hplib

    def launch():
        out = {}
        xl = x.clone().requires_grad_(True)
        y = ops.UpsampleAC.apply(xl, tuple(outs), None, 0.0)
        (out["dx"],) = torch.autograd.grad(y, [xl], dy)
        y2, yn = ops.UpsampleAC.apply(xl, tuple(outs), noise, amp)
        (out["dx2"],) = torch.autograd.grad([y2, yn], [xl], [dy, dy2])
        st.call = call0
        y3, yn3 = ops.UpsampleACNoise.apply(xl, tuple(outs), amp, first_noisy)
        (out["dx3"],) = torch.autograd.grad([y3, yn3], [xl], [dy, dy2])
        nz = torch.empty(B, C, *outs, device=DEV)
        hplib.call("hpvg_normal_f32", hplib.ptr(nz), ctypes.c_long(nz.numel()), ops._seed(), ctypes.c_uint(call0),
                   hplib.ptr(st.iter_dev), hplib.stream())
        out.update(y=y.detach(), y2=y2.detach(), yn=yn.detach(), y3=y3.detach(), yn3=yn3.detach(), nz=nz)
        torch.cuda.synchronize()
        return out

    o = launch()
    key = "%dd" % len(ins)
    yref, yA, ynref, ynA = E.resize64(x, outs, noise, amp)
    _check(o["y"], yref, yA, tag + "y", "resize.fwd", key)
    assert torch.equal(o["y2"], o["y"]), tag + "y differs between the launches with and without a noise tensor"
    _check(o["y3"], yref, yA, tag + "y of the noise-generating kernel", "resize.fwd.noisegen", key)
    _check(o["yn"], ynref, ynA, tag + "y + amp*noise", "resize.fwd.noise", key)
    _, _, yn3ref, yn3A = E.resize64(x, outs, o["nz"], amp)
    _check(o["yn3"][first_noisy:], yn3ref[first_noisy:], yn3A[first_noisy:], tag + "y + amp*N(0,1) in the kernel",
           "resize.fwd.noisegen", key)
    assert torch.equal(o["yn3"][:first_noisy], o["y3"][:first_noisy]), tag + "noise below first_noisy"
    del yref, yA, ynref, ynA, yn3ref, yn3A
    dref, dA = E.resize_bwd64(dy, ins)
    _check(o["dx"], dref, dA, tag + "dx", "resize.bwd", key)
    dref, dA = E.resize_bwd64(dy, ins, dy2)
    _check(o["dx2"], dref, dA, tag + "dx from dy + dy2", "resize.bwd.dy2", key)
    assert torch.equal(o["dx3"], o["dx2"]), tag + "UpsampleACNoise's backward differs from UpsampleAC's"


# ------------------------------------------------------------------------------------------------ penalty and losses
LOSS_CASES = [(cfg, lvl, sp) for cfg, shapes in R.level_shapes().items() for lvl, sp in enumerate(shapes)]


@pytest.mark.parametrize("cfg,lvl,sp", LOSS_CASES, ids=["%s-s%d" % (c[0], c[1]) for c in LOSS_CASES])
def test_penalty_and_losses_against_float64(ops, lib, cfg, lvl, sp):
    """Gradient penalty on (2, 3, level) gradients (lambda = 0.1, one voxel of zero norm), MSE on (2, 3, level), the critic
    terms on (2, 1, level), sqsum on a (2, 64, level) activation, KL at (2, 128, level 0)."""
    tag = "%s level %d %s: " % (cfg, lvl, tuple(sp))
    g = _gen(zlib.crc32(repr(("loss", cfg, lvl)).encode()))
    B, lam = 2, 0.1
    gr = 0.7 * torch.randn(B, 3, *sp, generator=g, device=DEV)
    gr[1, :, 0, 0] = 0
    a = torch.randn(B, 3, *sp, generator=g, device=DEV)
    b = torch.randn(B, 3, *sp, generator=g, device=DEV)
    d = torch.randn(B, 1, *sp, generator=g, device=DEV)
    act = torch.randn(B, E.BN_C, *sp, generator=g, device=DEV)
    lat = R.level_shapes()[cfg][0]
    mu = torch.randn(B, 128, *lat, generator=g, device=DEV)
    lv = 0.5 * torch.randn(B, 128, *lat, generator=g, device=DEV)
    gout = torch.tensor(0.83, device=DEV)

    def launch():
        out = {}
        gl, al, dl = gr.clone().requires_grad_(True), a.clone().requires_grad_(True), d.clone().requires_grad_(True)
        P = ops.GradPenalty.apply(gl, lam)
        (out["gp_bwd"],) = torch.autograd.grad(P, [gl], gout)
        m = ops.MSE.apply(al, b)
        (out["mse_bwd"],) = torch.autograd.grad(m, [al], gout)
        ms = ops.MeanScaled.apply(dl, -1.0)
        (out["ms_bwd"],) = torch.autograd.grad(ms, [dl], gout)
        mul, lvl_ = mu.clone().requires_grad_(True), lv.clone().requires_grad_(True)
        k = ops.KL.apply(mul, lvl_)
        out["kl_dmu"], out["kl_dlv"] = torch.autograd.grad(k, [mul, lvl_], gout)
        out.update(gp=P.detach(), mse=m.detach(), ms=ms.detach(), kl=k.detach(), sq=ops.sqsum(act.view(-1)))
        torch.cuda.synchronize()
        return out

    o = launch()
    key = "%dd" % len(sp)
    _check_scalar(o["gp"], *E.gp64(gr, lam), tag + "gradient penalty", "gp.fwd", key)
    _check(o["gp_bwd"], *E.gp_bwd64(float(gout), gr, lam), tag + "gradient penalty backward", "gp.bwd", key)
    assert float(o["gp_bwd"][1, :, 0, 0].abs().max()) == 0.0
    _check_scalar(o["mse"], *E.mse64(a, b), tag + "MSE", "mse.fwd", key)
    _check(o["mse_bwd"], *E.mse_bwd64(float(gout), a, b), tag + "MSE backward", "mse.bwd", key)
    _check_scalar(o["ms"], *E.mean_scaled64(d, -1.0), tag + "mean-scaled", "meanscaled.fwd", key)
    coef = torch.full_like(d, -1.0 / d.numel(), dtype=torch.float64) * float(gout)
    _check(o["ms_bwd"], coef, coef.abs(), tag + "mean-scaled backward", "meanscaled.bwd", key)
    _check_scalar(o["sq"], *E.sqsum64(act), tag + "sqsum", "sqsum", key)
    _check_scalar(o["kl"], *E.kl64(mu, lv), tag + "KL", "kl.fwd", key)
    (dm, dmA), (dl_, dlA) = E.kl_bwd64(float(gout), mu, lv)
    _check(o["kl_dmu"], dm, dmA, tag + "KL dmu", "kl.bwd", key)
    _check(o["kl_dlv"], dl_, dlA, tag + "KL dlogvar", "kl.bwd", key)
    _fill_ws(ops)
    _same(o, launch(), tag)
