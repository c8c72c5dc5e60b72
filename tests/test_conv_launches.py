"""Every conv launch the benchmark's pyramids make (tests/conv_ref.py launch_groups: video, video8 and image level shapes x
batch sizes 1, 2, 4 x the generator / critic / encoder / decoder layer shapes), at its real size, with the library's own size
rules, element by element against float64: |got - ref| <= TAU * A per element, A = the same operation on absolute values.

Per launch: the kernel kinds the size rules pick (the committed table of conv_ref.KINDS); forward with bias; forward with
LeakyReLU and the 1-bit mask words; backward-data plain, with a producer's 1-bit mask and with the fp32 mask; weight gradient
in overwrite and accumulate form and, where the library fuses it, with the bias gradient; the channel sum; and the same
launches again with every workspace byte set to 0xFF, which must reproduce the first results bit for bit (a launch that read
a workspace slot it did not write - a stream-K partial that was never stored - would not).

The launches of one (level shape, layer) share one weight tensor and one 4-sample input, walked at B = 2, 4, 1 (B < 4: the
first B samples), so the float64 reference is computed once per group, and the pack cache serves launches with and without
the two-axis section, as in training."""
import zlib

import pytest
import torch

import conv_ref as R
import launch_common as C

pytestmark = pytest.mark.gpu

DEV = "cuda"
CASES = [(cfg, lvl, layer, sp, B) for (cfg, lvl, layer, sp) in R.launch_groups() for B in R.BATCH_ORDER]
# worst |got - ref| / A per (quantity, kernel kind), printed at the end of the module
_STATS = {}
_GROUP = C.GroupCache()


def _id(case):
    cfg, lvl, (ci, co), sp, B = case
    return "%s-s%d-%dto%d-B%d" % (cfg, lvl, ci, co, B)


@pytest.fixture(scope="module")
def ops():
    import hp_vae_gan_amd  # noqa: F401
    from hp_vae_gan_amd import ops as _ops
    yield _ops
    _GROUP.clear()
    if _STATS:
        print("\nworst |got - ref| / A per (quantity, kernel kind), tau = %.0e:" % R.TAU)
        for (q, k), v in sorted(_STATS.items()):
            print("  %-16s kind %s  %.3e" % (q, k, v))


@pytest.fixture(scope="module")
def lib(ops):
    from hp_vae_gan_amd import lib as hplib
    return hplib.load()


def _group(key, layer, sp):
    """Inputs, weights and float64 references of one (level shape, layer), for the batch sizes of R.BATCHES."""
    return _GROUP.get_group(key, lambda: _make_group(key, layer, sp))


def _make_group(key, layer, sp):
    Ci, Co = layer
    nd = len(sp)
    n = max(R.BATCHES)
    g = torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))
    x = torch.randn(n, Ci, *sp, generator=g)
    dy = torch.randn(n, Co, *sp, generator=g)
    w = torch.randn(Co, Ci, *([3] * nd), generator=g) / (Ci * 3 ** nd) ** 0.5
    b = torch.randn(Co, generator=g)
    base = torch.randn(*w.shape, generator=g)
    bbase = torch.randn(Co, generator=g)
    y, yA = R.conv_fwd64(x, w, b)
    dx, dxA = R.conv_bwd_data64(dy, w)
    return dict(x=x.to(DEV), dy=dy.to(DEV), w=w.to(DEV), b=b.to(DEV), base=base.to(DEV), bbase=bbase.to(DEV),
                x_cpu=x, base64=base.double(), bbase64=bbase.double(), y=y, yA=yA, dx=dx, dxA=dxA,
                dw=R.conv_bwd_weight64(dy, x, w.shape, prefixes=R.BATCHES), db=R.bias_sum64(dy, prefixes=R.BATCHES))


def _check(got, ref, A, what, quantity, kind, **kw):
    C.checked(_STATS, got, ref, A, what, quantity, kind, **kw)


_decode_bits = C.decode_bits


@pytest.mark.parametrize("cfg,lvl,layer,sp,B", CASES, ids=[_id(c) for c in CASES])
def test_conv_launch_against_float64(ops, lib, cfg, lvl, layer, sp, B):
    Ci, Co = layer
    S = 1
    for v in sp:
        S *= v
    tag = "%s level %d %s %d->%d B=%d: " % (cfg, lvl, tuple(sp), Ci, Co, B)
    kinds = R.kinds_of(lib, B, layer, sp)
    assert kinds == R.expected_kinds(B, layer, sp), tag + "kernel kinds (fwd, bwd-data, wgrad, fuses_bias) %s" % (kinds,)
    kf, kd, kw, fb = kinds
    G = _group((cfg, lvl, layer, tuple(sp)), layer, sp)
    x, dy, w, b = G["x"][:B], G["dy"][:B], G["w"], G["b"]
    yref, yA, dxref, dxA = G["y"][:B], G["yA"][:B], G["dx"][:B], G["dxA"][:B]
    dwref, dwA = G["dw"][B]
    dbref, dbA = G["db"][B]
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
        bits = _decode_bits(r["ybits"], B, Co, S)
        assert torch.equal(bits, (r["ya"].cpu() > 0).view(B, Co, S)), tag + "mask words != the kernel's own y > 0"
        far = (yref.abs() > R.TAU * yA.double()).view(B, Co, S)
        assert torch.equal(bits[far], (yref > 0).view(B, Co, S)[far]), tag + "mask words != sign of the reference"
    _check(r["dx"], dxref, dxA, tag + "backward-data", "bwd", kd)
    f = torch.where(G["x_cpu"][:B] > 0, 1.0, 0.2).double()
    _check(r["dxf"], dxref * f, dxA * f, tag + "backward-data, fp32 mask", "bwd.out_mask", kd)
    if Ci > 4:
        _check(r["src"], R.lrelu(dxref), dxA, tag + "backward-data+lrelu", "bwd.lrelu", kd)
        m = _decode_bits(r["srcbits"], B, Ci, S)
        assert torch.equal(m, (r["src"].cpu() > 0).view(B, Ci, S)), tag + "producer's mask words != its own output > 0"
        f = torch.where(m, 1.0, 0.2).double().view(dxref.shape)
        _check(r["dxm"], dxref * f, dxA * f, tag + "backward-data, 1-bit mask", "bwd.mask_bits", kd)
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
