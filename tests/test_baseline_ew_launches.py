"""The BatchNorm, resize, pad / crop, add and tanh launches of the SinGAN-3D baselines config (bench.py --config baseline;
tests/ew_ref.py: baseline_bn_shapes, baseline_resize_launches) at their real sizes, B = 2, element by element against
float64, as tests/test_ew_launches.py holds the pyramids' launches: |got - ref| <= tau * A per element.

BatchNorm (C = 64, groups = 1, LeakyReLU on, as the baselines' ConvBlocks run it) at the cropped conv outputs level + 2 ...
+ 12 and the critic's level + 14: the plan of ew_ref.BASELINE_BN_PLANS, forward, statistics, running buffers, backward fresh
and direct-slot, and the rerun on a 0xFF-filled workspace.  Resize: GeneratorSG's 3-channel image to level + 14 with noise
made in the kernel, GeneratorCSG's 64-channel features to the level and, with in-kernel noise, to level + 10 (first_noisy =
0), forward and backward.  ops.ZeroPad (p = 7, 5, 1), ops.CropBorder and ops.Add bit for bit at every shape the generators
and the critic run them on.  ops.TanhRes forward and backward on (2, 3, level) of every level of all four configs."""
import ctypes
import zlib

import pytest
import torch
import torch.nn.functional as F

import conv_ref as R
import ew_ref as E
import launch_common as C

pytestmark = pytest.mark.gpu

DEV = "cuda"
B = R.BASELINE_B
_STATS = {}


@pytest.fixture(scope="module")
def ops():
    import hp_vae_gan_amd  # noqa: F401
    from hp_vae_gan_amd import ops as _ops
    yield _ops
    C.print_stats(_STATS, "baselines: worst |got - ref| / A per (op, path) (tau %.0e, statistics %.0e; tanh.fwd in units of "
                          "2^-24 |ref|, tanh.bwd of 2^-24 A):" % (E.TAU, E.TAU_STAT))


@pytest.fixture(scope="module")
def lib(ops):
    from hp_vae_gan_amd import lib as hplib
    return hplib.load()


def _check(got, ref, A, what, quantity, key, tau=E.TAU):
    C.checked(_STATS, got, ref, A, what, quantity, key, tau=tau)


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def _bits(t):
    return t.contiguous().view(torch.int32)


def _sid(sp):
    return "x".join(map(str, sp))


# ------------------------------------------------------------------------------------------------ BatchNorm
BN_CASES = E.baseline_bn_shapes()


@pytest.mark.parametrize("lvl,sp", BN_CASES, ids=["s%d-%s" % (l, _sid(s)) for l, s in BN_CASES])
def test_baseline_bn_launch_against_float64(ops, lib, lvl, sp):
    S = E.spatial(sp)
    plan = E.bn_plan_of(lib, B, S, 1)
    tag = "baseline level %d %s B=%d: " % (lvl, tuple(sp), B)
    assert plan == E.BASELINE_BN_PLANS[tuple(sp)], tag + "plan (fused, nsplit, V) %s" % (plan,)
    torch.cuda.empty_cache()
    g = _gen(_seed("bn", sp))
    Cn = E.BN_C
    one = (1, Cn, 1, 1, 1)
    r = torch.randn(B, Cn, *sp, generator=g, device=DEV) * (0.5 + torch.rand(one, generator=g, device=DEV)) \
        + (torch.rand(one, generator=g, device=DEV) * 2 - 1)
    dh = torch.randn(B, Cn, *sp, generator=g, device=DEV)
    gamma, beta = 1 + 0.3 * torch.randn(Cn, generator=g, device=DEV), 0.3 * torch.randn(Cn, generator=g, device=DEV)
    rm0, rv0 = 0.1 * torch.randn(Cn, generator=g, device=DEV), 1 + 0.2 * torch.rand(Cn, generator=g, device=DEV)
    base_g, base_b = torch.randn(Cn, generator=g, device=DEV), torch.randn(Cn, generator=g, device=DEV)
    pk = "%s V=%d" % ("fused" if plan[0] else "3-launch", plan[2])

    def launch():
        out = {}
        rm, rv = rm0.clone(), rv0.clone()
        rl = r.clone().requires_grad_(True)
        gl, bl = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
        h = ops.BNAct.apply(rl, gl, bl, rm, rv, E.BN_MOMENTUM, E.BN_EPS, True, 1)
        out["stats"] = h.grad_fn.saved_tensors[1].clone()
        out["dr"], out["dg"], out["db"] = torch.autograd.grad(h, [rl, gl, bl], dh, retain_graph=True)
        gl.grad, bl.grad = base_g.clone(), base_b.clone()
        h.backward(dh)
        out.update(h=h.detach(), rm=rm, rv=rv, dr_slot=rl.grad, dg_slot=gl.grad, db_slot=bl.grad)
        torch.cuda.synchronize()
        return out

    o = launch()
    ref = E.bn_fwd64(r, gamma, beta, rm0, rv0, groups=1, lrelu=True)
    _check(o["h"], *ref["h"], tag + "h", "bn.fwd.lrelu", pk)
    st = o["stats"]
    assert tuple(st.shape) == (1, 4, Cn)
    for j, name in enumerate(("mean", "invstd", "scale", "shift")):
        _check(st[:, j], *ref[name], tag + name, "bn.stat", pk, tau=E.TAU_STAT)
    _check(o["rm"], *ref["rm"], tag + "running_mean", "bn.running", pk, tau=E.TAU_STAT)
    _check(o["rv"], *ref["rv"], tag + "running_var", "bn.running", pk, tau=E.TAU_STAT)
    del ref
    bwd = E.bn_bwd64(dh, r, st, groups=1, lrelu=True)
    _check(o["dr"], *bwd["dr"], tag + "dr", "bn.bwd.lrelu", pk)
    _check(o["dg"], *bwd["dgamma"], tag + "dgamma", "bn.dgamma", pk)
    _check(o["db"], *bwd["dbeta"], tag + "dbeta", "bn.dbeta", pk)
    del bwd
    assert torch.equal(o["dr_slot"], o["dr"]), tag + "dr of the direct-slot backward differs"
    slot = E.bn_bwd64(dh, r, st, groups=1, lrelu=True, base_gamma=base_g, base_beta=base_b)
    _check(o["dg_slot"], *slot["dgamma"], tag + "dgamma, direct slot", "bn.dgamma.slot", pk)
    _check(o["db_slot"], *slot["dbeta"], tag + "dbeta, direct slot", "bn.dbeta.slot", pk)
    del slot
    C.fill_workspaces(ops)
    C.assert_same(o, launch(), tag)


# ------------------------------------------------------------------------------------------------ resize
RESIZE_CASES = E.baseline_resize_launches()


@pytest.mark.parametrize("lvl,Cn,ins,outs,noisy", RESIZE_CASES,
                         ids=["s%d-C%d-%s%s" % (c[0], c[1], _sid(c[3]), "-noise" if c[4] else "") for c in RESIZE_CASES])
def test_baseline_resize_launch_against_float64(ops, lib, lvl, Cn, ins, outs, noisy):
    """y against resize64; with in-kernel noise (UpsampleACNoise, first_noisy = 0, as the baselines generators call it) yn
    against y + amp * (what hpvg_normal_f32 writes for the same seed, call and iteration); backward against resize_bwd64
    with the gradient arriving through yn alone (the generators drop y), through y alone, and through both."""
    amp = 0.37
    tag = "baseline resize C=%d %s -> %s: " % (Cn, tuple(ins), tuple(outs))
    torch.cuda.empty_cache()
    g = _gen(_seed("resize", lvl, Cn, outs))
    x = torch.randn(B, Cn, *ins, generator=g, device=DEV)
    dy = torch.randn(B, Cn, *outs, generator=g, device=DEV)
    dy2 = torch.randn(B, Cn, *outs, generator=g, device=DEV)
    st = ops._rng(torch.device(DEV))
    call0 = 2000 + lvl
    from hp_vae_gan_amd import lib as hplib

    def launch():
        out = {}
        xl = x.clone().requires_grad_(True)
        y = ops.UpsampleAC.apply(xl, tuple(outs), None, 0.0)
        (out["dx"],) = torch.autograd.grad(y, [xl], dy)
        out["y"] = y.detach()
        if noisy:
            st.call = call0
            y3, yn3 = ops.UpsampleACNoise.apply(xl, tuple(outs), amp, 0)
            assert st.call == call0 + 1
            (out["dxn"],) = torch.autograd.grad([yn3], [xl], [dy2], retain_graph=True)
            (out["dx2"],) = torch.autograd.grad([y3, yn3], [xl], [dy, dy2])
            nz = torch.empty(B, Cn, *outs, device=DEV)
            hplib.call("hpvg_normal_f32", hplib.ptr(nz), ctypes.c_long(nz.numel()), ops._seed(), ctypes.c_uint(call0),
                       hplib.ptr(st.iter_dev), hplib.stream())
            out.update(y3=y3.detach(), yn3=yn3.detach(), nz=nz)
        torch.cuda.synchronize()
        return out

    o = launch()
    key = "C=%d" % Cn
    yref, yA = E.resize64(x, outs)
    _check(o["y"], yref, yA, tag + "y", "resize.fwd", key)
    if noisy:
        _check(o["y3"], yref, yA, tag + "y of the noise-generating kernel", "resize.fwd.noisegen", key)
        assert float(o["nz"].abs().max()) > 3.0 and abs(float(o["nz"].mean())) < 0.01, tag + "hpvg_normal_f32 wrote no N(0,1)"
        nzs = float(amp) * o["nz"].double()
        _check(o["yn3"], yref + nzs, yA + nzs.abs(), tag + "y + amp*N(0,1) in the kernel", "resize.fwd.noisegen", key)
        del nzs
    del yref, yA
    dref, dA = E.resize_bwd64(dy, ins)
    _check(o["dx"], dref, dA, tag + "dx", "resize.bwd", key)
    if noisy:
        dref, dA = E.resize_bwd64(dy2, ins)
        _check(o["dxn"], dref, dA, tag + "dx from the noisy output alone", "resize.bwd", key)
        dref, dA = E.resize_bwd64(dy, ins, dy2)
        _check(o["dx2"], dref, dA, tag + "dx from dy + dy2", "resize.bwd.dy2", key)
    second = launch()
    for k, v in o.items():
        assert torch.equal(second[k], v), tag + "%s is not reproduced by a second launch" % k


# ------------------------------------------------------------------------------------------------ pad, crop, add
def _rand(shape, seed):
    x = torch.randn(*shape, generator=_gen(seed), device=DEV)
    flat = x.view(-1)
    flat[::97] = -0.0                      # signs of zero and NaN payloads travel unchanged
    flat[5::101] = float("nan")
    return x


def _pad_ref(x, p):
    return F.pad(x, (p,) * 2 * (x.dim() - 2))


def _crop_ref(y, c):
    return y[(slice(None), slice(None)) + (slice(c, -c),) * (y.dim() - 2)].contiguous()


LEVELS = list(enumerate(R.baseline_level_shapes()))


@pytest.mark.parametrize("lvl,sp", LEVELS, ids=["s%d" % l for l, _ in LEVELS])
def test_baseline_pad_crop_add_bit_exact(ops, lvl, sp):
    """ops.ZeroPad with p = num_layer + 2 on (2, 3, level) (GeneratorSG's and the critic's input), p = num_layer on
    (2, 64, level) and p = 1 on (2, 64, level) and (2, 3, level) (GeneratorCSG's blocks, tail and head), each with its
    backward (CropBorder(p) of the padded shape); ops.CropBorder(1) of every generator conv output of the launch list with
    its backward (ZeroPad(1) of the cropped shape); ops.Add on (2, 3, level) and (2, 64, level): the bits of F.pad, slicing
    and fp32 a + b."""
    opt, shapes = R.baseline_opt()
    n, N, nc = int(opt.num_layer), int(opt.nfc), int(opt.nc_im)
    torch.cuda.empty_cache()
    for Cn, p in ((nc, n + 2), (N, n), (N, 1), (nc, 1)):
        tag = "level %d %s C=%d p=%d: " % (lvl, sp, Cn, p)
        x = _rand((B, Cn) + tuple(sp), _seed("pad", sp, Cn, p))
        y = ops.ZeroPad.apply(x, p)
        want = _pad_ref(x, p)
        assert y.shape == want.shape and torch.equal(_bits(y), _bits(want)), tag + "ZeroPad"
        assert torch.equal(_bits(ops.CropBorder.apply(y, p)), _bits(x)), tag + "CropBorder of the padded volume"
        big = _rand(tuple(want.shape), _seed("crop", sp, Cn, p))
        assert torch.equal(_bits(ops.CropBorder.apply(big, p)), _bits(_crop_ref(big, p))), tag + "CropBorder"
        del x, y, want, big
    seen = set()
    for net in ("GeneratorSG", "GeneratorCSG"):
        for (ci, co), shp in R.baseline_net_groups(net, lvl, opt, shapes):
            if (co, shp) in seen:
                continue
            seen.add((co, shp))
            tag = "level %d conv output C=%d %s: " % (lvl, co, shp)
            y = _rand((B, co) + tuple(shp), _seed("valid", shp, co))
            c = ops.CropBorder.apply(y, 1)
            want = _crop_ref(y, 1)
            assert c.shape == want.shape and torch.equal(_bits(c), _bits(want)), tag + "CropBorder(1)"
            assert torch.equal(_bits(ops.ZeroPad.apply(c, 1)), _bits(_pad_ref(want, 1))), tag + "ZeroPad(1) of the cropped volume"
            del y, c, want
    for Cn in (nc, N):
        a = _rand((B, Cn) + tuple(sp), _seed("add.a", sp, Cn))
        b = _rand((B, Cn) + tuple(sp), _seed("add.b", sp, Cn))
        got, want = ops.Add.apply(a, b), a + b
        nan = torch.isnan(want)
        assert torch.equal(torch.isnan(got), nan), "level %d Add C=%d: NaN positions" % (lvl, Cn)
        assert torch.equal(_bits(got)[~nan], _bits(want)[~nan]), "level %d Add C=%d" % (lvl, Cn)


# ------------------------------------------------------------------------------------------------ tanh
TANH_CASES = E.all_level_shapes()
U = E.U


def _units(got, ref):
    """max |got - ref| in units of 2^-24 * max(|ref|, 2^-126)."""
    return float(((got.double() - ref).abs() / (U * ref.abs().clamp_min(2.0 ** -126))).max())


@pytest.mark.parametrize("cfg,lvl,sp", TANH_CASES, ids=["%s-s%d" % (c[0], c[1]) for c in TANH_CASES])
@pytest.mark.parametrize("with_res", [False, True], ids=["nores", "res"])
def test_tanh_res_against_float64(ops, cfg, lvl, sp, with_res):
    """ops.TanhRes on (2, 3, level) of every level of the four configs: sample 0 holds N(0,1) data, sample 1 is spread
    evenly over [-6, 6]; res (present or absent) is 0.5 N(0,1).

    Forward: y against float64 tanh(x + res), in units of 2^-24 * max(|ref|, 2^-126).  The error of the device's tanhf is not
    written down in this project, so the bound comes from a second, independent implementation: torch.tanh in fp32 on the
    CPU, measured in the same units on the same inputs (with the same fp32 x + res), and the kernel may be 4x as far off: a
    1-2 ulp difference between two libm implementations of one function passes, a wrong x + res or a dropped tail element
    does not (the units are relative to |ref|: any element left unwritten or built from other inputs is off by >= 1e5
    units).  Measured on the CPU over all 54 cases (data of the same distribution): worst 2.04 units, hence a bound of at
    most 8.2 units; the bound of a case is 4x ITS CPU figure, which is printed, and a CPU figure above 4 units is refused.

    Backward: dx = dy * (1 - y*y) from the kernel's own fp32 y.  Three roundings - of y*y, of 1 - y*y (which also carries
    the first) and of the product - give |dx - ref| <= 2^-24 * A (1 + O(2^-24)), A = |dy| (y^2 + 2 |1 - y^2|); fused
    multiply-adds only drop terms.  tau = 1.001 * 2^-24."""
    tag = "%s level %d %s tanh%s: " % (cfg, lvl, tuple(sp), " + res" if with_res else "")
    g = _gen(_seed("tanh", cfg, lvl, with_res))
    n1 = 3 * E.spatial(sp)
    x = torch.empty(2, 3, *sp, device=DEV)
    x[0] = torch.randn(3, *sp, generator=g, device=DEV)
    x[1] = torch.linspace(-6.0, 6.0, n1, device=DEV)[torch.randperm(n1, generator=g, device=DEV)].view(3, *sp)
    res = 0.5 * torch.randn(2, 3, *sp, generator=g, device=DEV) if with_res else None
    dy = torch.randn(2, 3, *sp, generator=g, device=DEV)
    xl = x.clone().requires_grad_(True)
    rl = res.clone().requires_grad_(True) if with_res else None
    y = ops.TanhRes.apply(xl, rl)
    grads = torch.autograd.grad(y, [xl, rl] if with_res else [xl], dy)
    torch.cuda.synchronize()
    y = y.detach()

    s64 = x.double() + (res.double() if with_res else 0.0)
    ref = torch.tanh(s64)
    xc, rc = x.cpu(), (res.cpu() if with_res else None)
    cpu = torch.tanh(xc + rc if with_res else xc)
    cpu_units = _units(cpu, ref.cpu())
    got_units = _units(y, ref)
    print("%sCPU torch.tanh %.3f units, kernel %.3f units, bound %.3f" % (tag, cpu_units, got_units, 4 * cpu_units))
    k = ("tanh.fwd", "res" if with_res else "-")
    _STATS[k] = max(_STATS.get(k, 0.0), got_units)
    assert cpu_units <= 4.0, tag + "the CPU's own tanh is %.2f units off: no yardstick" % cpu_units
    assert got_units <= 4 * cpu_units, tag + "%.3f units of 2^-24 |ref| > 4 x the CPU's %.3f" % (got_units, cpu_units)
    assert bool((y.abs() <= 1).all())

    y64 = y.double()
    dref = dy.double() * (1 - y64 * y64)
    dA = dy.double().abs() * (y64 * y64 + 2 * (1 - y64 * y64).abs())
    r = R.check(grads[0], dref, dA, tag + "dx", tau=1.001 * U)
    k = ("tanh.bwd", "res" if with_res else "-")
    _STATS[k] = max(_STATS.get(k, 0.0), r / U)
    if with_res:
        assert torch.equal(grads[1], grads[0]), tag + "the residual's gradient is not dx"
