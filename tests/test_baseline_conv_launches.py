"""Every conv launch of the SinGAN-3D baselines config (tests/conv_ref.py baseline_launch_groups: GeneratorSG, GeneratorCSG
and WDiscriminatorBaselines over the eight levels of bench.py --config baseline, 81 (layer, padded shape) pairs, B = 2), at
its real size, with the library's own size rules, element by element against float64: |got - ref| <= TAU * A per element,
exactly as tests/test_conv_launches.py holds the pyramids' launches.

Per group: the kernel kinds the size rules pick (the committed table conv_ref.BASELINE_KINDS); forward with bias; forward
with LeakyReLU and the 1-bit mask words; backward-data plain, with the fp32 mask and with a producer's 1-bit mask; weight
gradient in overwrite and accumulate form and, where the library fuses it, with the bias gradient; the channel sum; and the
same launches again with every workspace byte set to 0xFF, which must reproduce the first results bit for bit.

Reference.  conv_ref's CPU functions need ~16 GB of im2col per sample at 64 x 27 x 158 x 270, so the references here are
conv_ref's tap-sum forms (conv_fwd64_taps, conv_bwd_data64_taps, conv_bwd_weight64_taps): float64 sums over the 27 taps of a
channel matmul on shifted views, run through torch's own matmul on the device.  They share no code with libhpvg;
tests/test_baseline_launch_host.py pins them against the CPU functions within 1e-12 of A.

The first test records a real train step to show that the launch list is the truth."""
import zlib

import pytest
import torch

import conv_ref as R
import launch_common as C

pytestmark = pytest.mark.gpu

DEV = "cuda"
B = R.BASELINE_B
CASES = R.baseline_launch_groups()
# worst |got - ref| / A per (quantity, kernel kind), printed at the end of the module
_STATS = {}
_GROUP = C.GroupCache()


def _id(case):
    _, lvl, (ci, co), sp = case
    return "s%d-%dto%d-%s" % (lvl, ci, co, "x".join(map(str, sp)))


@pytest.fixture(scope="module")
def ops():
    import hp_vae_gan_amd  # noqa: F401
    from hp_vae_gan_amd import ops as _ops
    yield _ops
    _GROUP.clear()
    C.print_stats(_STATS, "baselines: worst |got - ref| / A per (quantity, kernel kind), tau = %.0e:" % R.TAU)


@pytest.fixture(scope="module")
def lib(ops):
    from hp_vae_gan_amd import lib as hplib
    return hplib.load()


# ------------------------------------------------------------------------------------------------ the list is the truth
STEPS = [(g, d, s) for g, d in (("GeneratorSG", "WDiscriminator3D"), ("GeneratorCSG", "WDiscriminator3D"),
                                ("GeneratorSG", "WDiscriminatorBaselines")) for s in (0, 2)]


@pytest.mark.parametrize("generator,discriminator,stage", STEPS, ids=["%s-%s-s%d" % c for c in STEPS])
def test_recorded_step_launches_equal_the_list(ops, generator, discriminator, stage):
    """One eager BaselineStageTrainer.step at the bench geometry with every conv and weight-gradient launch recorded
    (ops.KernelTimer): each recorded (B, Cin, Cout, T, H, W) - a forward view, the flipped view of a backward-data conv or a
    weight gradient - is a B = 2 launch of one (layer, shape), and the set of those equals conv_ref.baseline_step_groups:
    entries of baseline_launch_groups() plus, for WDiscriminator3D, the unpadded critic shapes of launch_groups()."""
    import copy
    from hp_vae_gan_amd import train as hp_train
    from hp_vae_gan_amd.modules import networks_3d
    torch.manual_seed(0)
    opt, shapes = R.baseline_opt(DEV, generator=generator, discriminator=discriminator)
    proto = getattr(networks_3d, generator)(opt)
    for _ in range(stage):
        proto.init_next_stage()
    opt.scale_idx = stage
    opt.Noise_Amps = [1] + [0.05] * max(0, stage - 1)
    netG = copy.deepcopy(proto).to(DEV)
    netG.opt = opt
    g = torch.Generator().manual_seed(100 + stage)
    real = (torch.rand(opt.batch_size, 3, *shapes[stage], generator=g) * 2 - 1).to(DEV)
    opt.Z_init = torch.randn(opt.batch_size, 3, *shapes[0], generator=torch.Generator().manual_seed(99)).to(DEV)
    trainer = hp_train.BaselineStageTrainer(opt, netG)
    assert type(trainer.netD).__name__.startswith(discriminator.replace("3D", ""))

    def match(desc):
        if desc["KT"] != 3:
            return "other"
        return "wgrad" if desc["op"] == "wgrad" else ("flip" if desc["flip"] else "fwd")

    timer = ops.KernelTimer(match)
    ops.set_kernel_timer(timer)
    try:
        trainer.step(real)
        torch.cuda.synchronize()
    finally:
        ops.set_kernel_timer(None)
    seen = {"fwd": set(), "flip": set(), "wgrad": set()}
    for (fam, b, ci, co, T, H, W), _, _ in timer.events:
        assert fam != "other" and b == B, (fam, b, ci, co, T, H, W)
        seen[fam].add(((co, ci) if fam == "flip" else (ci, co), (T, H, W)))   # the layer a flipped launch belongs to
    want = R.baseline_step_groups(generator, discriminator, stage)
    got = seen["fwd"] | seen["flip"] | seen["wgrad"]
    assert got == want, "recorded but not listed: %s; listed but not recorded: %s" % (sorted(got - want), sorted(want - got))
    assert seen["fwd"] == want, "every listed layer runs forward: %s" % sorted(want - seen["fwd"])
    listed = set((c[2], c[3]) for c in CASES) | set((c[2], c[3]) for c in R.launch_groups())
    assert got <= listed
    assert seen["flip"] and seen["wgrad"]


# ------------------------------------------------------------------------------------------------ the launches
def _group(key, layer, sp):
    """Inputs, weights and float64 references (on the device) of one (layer, padded shape) at B = 2."""
    return _GROUP.get_group(key, lambda: _make_group(key, layer, sp))


def _make_group(key, layer, sp):
    torch.cuda.empty_cache()
    Ci, Co = layer
    g = torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))
    x = torch.randn(B, Ci, *sp, generator=g).to(DEV)
    dy = torch.randn(B, Co, *sp, generator=g).to(DEV)
    w = (torch.randn(Co, Ci, 3, 3, 3, generator=g) / (Ci * 27) ** 0.5).to(DEV)
    b = torch.randn(Co, generator=g).to(DEV)
    base = torch.randn(*w.shape, generator=g).to(DEV)
    bbase = torch.randn(Co, generator=g).to(DEV)
    y, yA = R.conv_fwd64_taps(x, w, b)
    dx, dxA = R.conv_bwd_data64_taps(dy, w)
    return dict(x=x, dy=dy, w=w, b=b, base=base, bbase=bbase, base64=base.double(), bbase64=bbase.double(), y=y, yA=yA,
                dx=dx, dxA=dxA, dw=R.conv_bwd_weight64_taps(dy, x), db=R.bias_sum64_on(dy))


def _check(got, ref, A, what, quantity, kind, **kw):
    C.checked(_STATS, got, ref, A, what, quantity, kind, **kw)


@pytest.mark.parametrize("cfg,lvl,layer,sp", CASES, ids=[_id(c) for c in CASES])
def test_baseline_conv_launch_against_float64(ops, lib, cfg, lvl, layer, sp):
    Ci, Co = layer
    S = sp[0] * sp[1] * sp[2]
    tag = "baseline level %d %s %d->%d B=%d: " % (lvl, tuple(sp), Ci, Co, B)
    kinds = R.kinds_of(lib, B, layer, sp)
    assert kinds == R.baseline_expected_kinds(layer, sp), tag + "kernel kinds (fwd, bwd-data, wgrad, fuses_bias) %s" % (kinds,)
    kf, kd, kw, fb = kinds
    G = _group((cfg, lvl, layer, tuple(sp)), layer, sp)
    x, dy, w, b = G["x"], G["dy"], G["w"], G["b"]
    yref, yA, dxref, dxA = G["y"], G["yA"], G["dx"], G["dxA"]
    dwref, dwA = G["dw"]
    dbref, dbA = G["db"]
    wn = R.WEIGHT_NAMES[w.dim()]

    def launch():
        out = {"y": ops.conv_fwd_raw(x, w, b), "dx": ops.conv_fwd_raw(dy, w, None, flip=True),
               "dxf": ops.conv_fwd_raw(dy, w, None, flip=True, out_mask=x)}
        if Co > 4:
            out["ya"], out["ybits"] = ops.conv_fwd_raw(x, w, b, out_lrelu=True, want_bits=True)
        if Ci > 4:   # a producer of dx's shape writes the 1-bit mask the masked backward-data launch reads
            out["src"], out["srcbits"] = ops.conv_fwd_raw(dy, w, None, flip=True, out_lrelu=True, want_bits=True)
            out["dxm"] = ops.conv_fwd_raw(dy, w, None, flip=True, mask_bits=out["srcbits"])
        out["dw"] = ops.conv_bwd_weight_raw(dy, x, w.shape)
        out["acc"] = G["base"].clone()
        assert ops.conv_bwd_weight_raw(dy, x, w.shape, into=out["acc"]) is None
        out["accw"], out["accb"] = G["base"].clone(), G["bbase"].clone()
        out["fused"] = ops.conv_bwd_weight_bias_raw(dy, x, w.shape, out["accw"], out["accb"])
        out["db"] = ops.channel_sum_raw(dy)
        torch.cuda.synchronize()
        return out

    r = launch()
    _check(r["y"], yref, yA, tag + "forward", "fwd", kf)
    if Co > 4:
        _check(r["ya"], R.lrelu(yref), yA, tag + "forward+lrelu", "fwd.lrelu", kf)
        bits = C.decode_bits(r["ybits"], B, Co, S, DEV)
        assert torch.equal(bits, (r["ya"] > 0).view(B, Co, S)), tag + "mask words != the kernel's own y > 0"
        far = (yref.abs() > R.TAU * yA.double()).view(B, Co, S)
        assert torch.equal(bits[far], (yref > 0).view(B, Co, S)[far]), tag + "mask words != sign of the reference"
        del bits, far
    _check(r["dx"], dxref, dxA, tag + "backward-data", "bwd", kd)
    f = torch.where(x > 0, 1.0, 0.2).double()
    _check(r["dxf"], dxref * f, dxA * f, tag + "backward-data, fp32 mask", "bwd.out_mask", kd)
    if Ci > 4:
        _check(r["src"], R.lrelu(dxref), dxA, tag + "backward-data+lrelu", "bwd.lrelu", kd)
        m = C.decode_bits(r["srcbits"], B, Ci, S, DEV)
        assert torch.equal(m, (r["src"] > 0).view(B, Ci, S)), tag + "producer's mask words != its own output > 0"
        f = torch.where(m, 1.0, 0.2).double().view(dxref.shape)
        del m
        _check(r["dxm"], dxref * f, dxA * f, tag + "backward-data, 1-bit mask", "bwd.mask_bits", kd)
    del f
    _check(r["dw"], dwref, dwA, tag + "weight gradient", "wgrad", kw, names=wn)
    _check(r["acc"], G["base64"] + dwref, G["base64"].abs().float() + dwA, tag + "weight gradient, accumulate", "wgrad.acc", kw,
           names=wn)
    assert r["fused"] == bool(fb), tag + "fused weight + bias launch %s, fuses_bias %d" % (r["fused"], fb)
    if r["fused"]:
        _check(r["accw"], G["base64"] + dwref, G["base64"].abs().float() + dwA, tag + "fused weight gradient", "wgrad.fused", kw,
               names=wn)
        _check(r["accb"], G["bbase64"] + dbref, G["bbase64"].abs().float() + dbA, tag + "fused bias gradient", "bias.fused", kw)
        assert torch.equal(r["accw"], r["acc"]), tag + "the fused launch's weight gradient differs from the plain launch's"
    _check(r["db"], dbref, dbA, tag + "channel sum", "bias.sum", "-")

    # the same launches on a workspace full of NaN (0xFF bytes): every slot a launch reads it must have written itself
    C.fill_workspaces(ops)
    C.assert_same(r, launch(), tag)
