"""Launches on tensors at any 4-byte offset, inside guard bands (tests/offset_buf.py).

The other launch suites hand every kernel fresh allocations: 256-byte aligned starts, followed by allocator slack nobody looks
at.  Training does not: ops.SplitBatch returns x[n:] (the critic's input `fake` starts B*3*T*H*W floats into the merged batch),
Concat2.backward returns g[n:], concat_batch writes out[o:o+n], and lib.ptr() asks for contiguity alone.  The contract at the
top of include/hpvg.h says 4-byte alignment is enough and nothing outside [p, p + n) is touched; this module enforces it.

Common rule.  Every launch runs once with all tensors at offset 0 in guard bands (the base), once with each tensor argument in
turn at offset 1, 2, 3 elements past a 16-byte boundary, and once with all of them at 1.  Inputs sit between NaN guards (-1
for mask words), outputs are out_like buffers (sentinel bits in guards and payload) wherever the C ABI takes the output
pointer - those launches call the library directly.  After every launch every output's guards are bit-intact, no output element
is NaN or still the sentinel, and no input's guard was written.

(a) convolutions: no conv kernel looks at the pointer value, so every offset launch equals the base bit for bit; the base is
    checked against float64 (conv_ref.check, TAU, the A bounds of conv_ref).  Default size rules and the forced kernel families;
    the kinds reached must cover conv_ref.KINDS.
(b) BatchNorm family and channel sum: the vector width comes from the pointer (hpvg_vec_width_at); launches of one case with the
    same width are bit-equal, every launch is checked against float64 (ew_ref, TAU / TAU_STAT); V = 4, 2, 1 must each be
    chosen by the pointer on an S % 4 == 0 shape.
(c) pointwise, losses, resize, copies, the variant models' kernels (csrc/variants.hip): bit-equal to the base, base against
    float64 where ew_ref / variant_ref has a reference.
(d) the producer itself: one critic step on SplitBatch's `fake` and on fake.clone() agree bit for bit.

The module prints, per section, the launches compared bit for bit, the launches compared with float64 and the worst
|got - ref| / A per (op, path)."""
import contextlib
import ctypes
import types
import zlib

import pytest
import torch
import torch.nn.functional as F

import conv_ref as R
import ew_ref as E
import launch_common as LC
import offset_buf as OB
from helpers import RTOL, assert_close

pytestmark = pytest.mark.gpu

DEV = "cuda"
_STATS = {"a": {}, "b": {}, "c": {}}
_COUNT = {s: {"bit": 0, "f64": 0, "launches": 0} for s in "abcd"}
_FWD_KINDS, _WGRAD_KINDS = set(), set()      # kernel kinds the conv launches reached
_V_BY_POINTER = set()                        # vector widths seen on S % 4 == 0 shapes (4 aligned, 2 / 1 through the offset)
_BOX_FORMS = set()
_RAN = {"conv": set(), "bn": set(), "box": set()}


@pytest.fixture(scope="module")
def ops():
    import hp_vae_gan_amd  # noqa: F401
    from hp_vae_gan_amd import ops as _ops
    yield _ops
    _ops.weights_changed()
    for sec, title in (("a", "convolutions"), ("b", "BatchNorm family, channel sum"), ("c", "pointwise, losses, resize, copies"),
                       ("d", "the producer")):
        c = _COUNT[sec]
        print("\n(%s) %s: %d launches, %d compared bit for bit, %d compared with float64" % (sec, title, c["launches"], c["bit"],
                                                                                           c["f64"]))
        if _STATS.get(sec):
            LC.print_stats(_STATS[sec], "    worst |got - ref| / A per (op, path), tau %.0e (statistics %.0e):" % (E.TAU, E.TAU_STAT))


@pytest.fixture(scope="module")
def hplib(ops):
    from hp_vae_gan_amd import lib as _hplib
    _hplib.load()
    return _hplib


@pytest.fixture(scope="module")
def lib(hplib):
    return hplib.load()


def _gen(*key):
    return torch.Generator(device=DEV).manual_seed(zlib.crc32(repr(key).encode()))


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, device=DEV)


# ------------------------------------------------------------------------------------------------ the common rule
def _configs(names):
    yield "base", {}
    for n in names:
        for off in (1, 2, 3):
            yield "%s@%d" % (n, off), {n: off}
    yield "all@1", {n: 1 for n in names}


def sweep(sec, what, ins, outs, run, vary=None, guards=None, configs=None):
    """The common rule for one launch.  ins: {name: tensor or None}; outs: {name: (shape, dtype, initial payload or None)};
    run(T) launches on the dict of placed tensors and may return further results ({name: tensor}, allocated by ops).  vary: the
    names that take offsets (default: all).  Returns [(label, placed tensors, results)]; results hold the out_like views and
    whatever run returned."""
    guards = guards or {}
    names = list(vary) if vary is not None else [n for n, t in ins.items() if t is not None] + list(outs)
    done = []
    for label, offs in (configs if configs is not None else _configs(names)):
        T = {}
        for n, t in ins.items():
            T[n] = None if t is None else OB.embed(t, offs.get(n, 0), guard=guards.get(n))
        for n, (shape, dtype, init) in outs.items():
            T[n] = OB.out_like(shape, dtype, offs.get(n, 0), guard=guards.get(n), device=DEV)
            if init is not None:
                T[n].copy_(init)
        extra = run(T) or {}
        torch.cuda.synchronize()
        tag = "%s [%s]" % (what, label)
        for n in outs:
            OB.assert_written(T[n], tag + " output " + n)
        for n, t in ins.items():
            if t is not None:
                assert OB.guards_intact(T[n]), tag + ": the guard band of input %s was written" % n
        res = {n: T[n] for n in outs}
        for n, t in extra.items():
            assert not bool(torch.isnan(t).any()), tag + ": NaN in %s (a guard value of an input was read)" % n
            res[n] = t
        done.append((label, T, res))
        _COUNT[sec]["launches"] += 1
    return done


def all_equal(sec, done, what, ref=0):
    """Every launch of a sweep equals launch `ref` (the base) bit for bit, in every result."""
    base = done[ref][2]
    for label, _, res in done:
        if res is base:
            continue
        for n, t in base.items():
            assert torch.equal(res[n], t), "%s [%s]: %s differs from the %s launch" % (what, label, n, done[ref][0])
        _COUNT[sec]["bit"] += 1
    return base


def check(sec, got, ref, A, what, quantity, key, tau=E.TAU, **kw):
    LC.checked(_STATS[sec], got, ref, A, what, quantity, key, tau=tau, **kw)
    _COUNT[sec]["f64"] += 1


def check_scalar(sec, got, ref, A, what, quantity, key):
    check(sec, got.reshape(1), ref.reshape(1), A.reshape(1).float(), what, quantity, key)


# ================================================================================================ (a) convolutions
# (B, (Cin, Cout), shape): the smallest shapes at which each staging form still has its edge cases (tests/test_hip_ops.py
# argues for each)
CONV_CASES = [
    (1, (64, 64), (2, 5, 7)),        # odd W, H*W = 3 (mod 4)
    (1, (64, 64), (3, 57, 102)),     # H*W = 2 (mod 4), several tiles per plane, plane-end patch
    (2, (16, 40), (2, 3, 2)),        # W = 2, ragged channels
    (2, (64, 64), (2, 4, 6)),        # H*W = 0 (mod 4)
    (1, (24, 40), (2, 3, 3)),
    (2, (3, 64), (5, 7, 9)),         # heads and tails
    (2, (64, 3), (3, 6, 5)),
    (2, (64, 1), (2, 5, 7)),
    (2, (3, 64), (11, 13)),          # 2-D
    (2, (64, 64), (9, 10)),
    (2, (64, 3), (30, 41)),
]
FWD_MODES = (None, 0, 3, 4, 5)        # None: the default size rules; hpvg_conv_wino_config modes
WGRAD_MODES = (None, 0, 2, 3, 4, 5)   # hpvg_conv_bwd_weight_wino_config modes


def _conv_id(c):
    B, (ci, co), sp = c
    return "%dto%d-%s-B%d" % (ci, co, "x".join(map(str, sp)), B)


@contextlib.contextmanager
def fwd_mode(lib, mode):
    prev = lib.hpvg_conv_wino_config(-1, -1)
    try:
        if mode is not None:
            assert lib.hpvg_conv_wino_config(mode, -1) == mode
        yield
    finally:
        lib.hpvg_conv_wino_config(prev, -1)


@contextlib.contextmanager
def wgrad_mode(lib, mode):
    prev = lib.hpvg_conv_bwd_weight_wino_config(-1)
    try:
        if mode is not None:
            assert lib.hpvg_conv_bwd_weight_wino_config(mode) == mode
        yield
    finally:
        lib.hpvg_conv_bwd_weight_wino_config(prev)


def _conv_launch(ops, hplib, T, view, Ci_l, Co_l, flip, out_lrelu=False):
    """hpvg_conv_fwd_f32 / hpvg_conv_fwd_bits_f32 on the placed tensors of T: x, w, bias, y and optionally out_mask, mask_bits,
    bits (as ops.conv_fwd_raw launches them, with the output pointers ours)."""
    B, Tt, H, W, KT = view
    cin_k, cout_k = (Co_l, Ci_l) if flip else (Ci_l, Co_l)
    wp = ops.pack_weight(T["w"], flip, (B, Tt, H, W))
    nws = hplib.call("hpvg_conv_fwd_ws_bytes", B, cin_k, cout_k, Tt, H, W, KT)
    ws = ops._scratch(nws, T["x"].device) if nws else (None, 0)
    p = hplib.ptr
    if T.get("bits") is not None or T.get("mask_bits") is not None:
        hplib.call("hpvg_conv_fwd_bits_f32", p(T["x"]), p(wp), p(T.get("bias")), p(T["y"]), 1 if out_lrelu else 0, p(T.get("mask_bits")),
                   p(T.get("bits")), *ws, B, cin_k, cout_k, Tt, H, W, KT, hplib.stream())
    else:
        hplib.call("hpvg_conv_fwd_f32", p(T["x"]), p(wp), p(T.get("bias")), None, None, 0, p(T["y"]), 1 if out_lrelu else 0,
                   p(T.get("out_mask")), *ws, B, cin_k, cout_k, Tt, H, W, KT, hplib.stream())


def _conv_group(B, layer, sp):
    Ci, Co = layer
    nd = len(sp)
    g = torch.Generator().manual_seed(zlib.crc32(repr(("offset", B, layer, sp)).encode()))
    x = torch.randn(B, Ci, *sp, generator=g)
    dy = torch.randn(B, Co, *sp, generator=g)
    w = torch.randn(Co, Ci, *([3] * nd), generator=g) / (Ci * 3 ** nd) ** 0.5
    b = torch.randn(Co, generator=g)
    base = torch.randn(*w.shape, generator=g)
    bbase = torch.randn(Co, generator=g)
    G = dict(x=x.to(DEV), dy=dy.to(DEV), w=w.to(DEV), b=b.to(DEV), base=base.to(DEV), bbase=bbase.to(DEV), x_cpu=x,
             base64=base.double(), bbase64=bbase.double())
    G["y0"], G["y0A"] = R.conv_fwd64(x, w, None)
    G["y"], G["yA"] = R.conv_fwd64(x, w, b)
    G["dx"], G["dxA"] = R.conv_bwd_data64(dy, w)
    G["dw"], G["dwA"] = R.conv_bwd_weight64(dy, x, w.shape)
    G["db"], G["dbA"] = R.bias_sum64(dy)
    return G


@pytest.mark.parametrize("B,layer,sp", CONV_CASES, ids=[_conv_id(c) for c in CONV_CASES])
def test_conv_launches_at_every_offset(ops, hplib, lib, B, layer, sp):
    Ci, Co = layer
    T_, H, W, KT = R.kernel_view(sp)
    view = (B, T_, H, W, KT)
    S = T_ * H * W
    tag = "%d->%d %s B=%d" % (Ci, Co, tuple(sp), B)
    G = _conv_group(B, layer, sp)
    x, dy, w, b = G["x"], G["dy"], G["w"], G["b"]
    xs, ys = tuple(x.shape), tuple(dy.shape)
    wn = R.WEIGHT_NAMES[w.dim()]
    f32, i32 = torch.float32, torch.int32
    act_guard = {"bits": OB.guard_for(xs), "mask_bits": OB.guard_for(xs)}

    for mode in FWD_MODES:
        with fwd_mode(lib, mode):
            kf = lib.hpvg_conv_fwd_kernel_kind(B, Ci, Co, T_, H, W, KT)
            kd = lib.hpvg_conv_fwd_kernel_kind(B, Co, Ci, T_, H, W, KT)
            assert kf >= 0 and kd >= 0
            _FWD_KINDS.update((kf, kd))
            mt = "%s mode %s: " % (tag, mode)

            def fwd(T, lrelu=False):
                _conv_launch(ops, hplib, T, view, Ci, Co, False, out_lrelu=lrelu)

            def bwd(T, lrelu=False):
                _conv_launch(ops, hplib, T, view, Ci, Co, True, out_lrelu=lrelu)

            r = all_equal("a", sweep("a", mt + "forward", {"x": x, "w": w}, {"y": (ys, f32, None)}, fwd), mt + "forward")
            check("a", r["y"], G["y0"], G["y0A"], mt + "forward", "fwd", kf)
            r = all_equal("a", sweep("a", mt + "forward+bias", {"x": x, "w": w, "bias": b}, {"y": (ys, f32, None)}, fwd),
                          mt + "forward+bias")
            check("a", r["y"], G["y"], G["yA"], mt + "forward+bias", "fwd.bias", kf)
            if Co > 4:
                nw = hplib.call("hpvg_conv_mask_words", B, Co, T_, H, W)
                r = all_equal("a", sweep("a", mt + "forward+lrelu+bits", {"x": x, "w": w, "bias": b},
                                         {"y": (ys, f32, None), "bits": ((nw,), i32, None)}, lambda T: fwd(T, True), guards=act_guard),
                              mt + "forward+lrelu+bits")
                check("a", r["y"], R.lrelu(G["y"]), G["yA"], mt + "forward+lrelu", "fwd.lrelu", kf)
                bits = LC.decode_bits(r["bits"].contiguous(), B, Co, S)
                assert torch.equal(bits, (r["y"].cpu() > 0).view(B, Co, S)), mt + "mask words != the kernel's own y > 0"
            r = all_equal("a", sweep("a", mt + "backward-data", {"x": dy, "w": w}, {"y": (xs, f32, None)}, bwd), mt + "backward-data")
            check("a", r["y"], G["dx"], G["dxA"], mt + "backward-data", "bwd", kd)
            # the fp32 mask is a tensor argument of its own: it takes its turn at being offset
            r = all_equal("a", sweep("a", mt + "backward-data, fp32 mask", {"x": dy, "w": w, "out_mask": x}, {"y": (xs, f32, None)}, bwd),
                          mt + "backward-data, fp32 mask")
            fm = torch.where(G["x_cpu"] > 0, 1.0, 0.2).double()
            check("a", r["y"], G["dx"] * fm, G["dxA"] * fm, mt + "backward-data, fp32 mask", "bwd.out_mask", kd)
            if Ci > 4:
                # a producer of dx's shape writes the 1-bit mask the masked backward-data launch reads
                nw = hplib.call("hpvg_conv_mask_words", B, Ci, T_, H, W)
                r = all_equal("a", sweep("a", mt + "backward-data+lrelu+bits", {"x": dy, "w": w},
                                         {"y": (xs, f32, None), "bits": ((nw,), i32, None)}, lambda T: bwd(T, True), guards=act_guard),
                              mt + "backward-data+lrelu+bits")
                check("a", r["y"], R.lrelu(G["dx"]), G["dxA"], mt + "backward-data+lrelu", "bwd.lrelu", kd)
                srcbits = r["bits"].clone()
                m = LC.decode_bits(srcbits, B, Ci, S)
                assert torch.equal(m, (r["y"].cpu() > 0).view(B, Ci, S)), mt + "producer's mask words != its own output > 0"
                r = all_equal("a", sweep("a", mt + "backward-data, 1-bit mask", {"x": dy, "w": w, "mask_bits": srcbits},
                                         {"y": (xs, f32, None)}, bwd, guards=act_guard), mt + "backward-data, 1-bit mask")
                fb = torch.where(m, 1.0, 0.2).double().view(G["dx"].shape)
                check("a", r["y"], G["dx"] * fb, G["dxA"] * fb, mt + "backward-data, 1-bit mask", "bwd.mask_bits", kd)
            ops.weights_changed()

    wsh = tuple(w.shape)
    p = hplib.ptr
    for mode in WGRAD_MODES:
        with wgrad_mode(lib, mode):
            kw = lib.hpvg_conv_bwd_weight_kernel_kind(B, Ci, Co, T_, H, W, KT)
            fuses = lib.hpvg_conv_bwd_weight_fuses_bias(B, Ci, Co, T_, H, W, KT)
            assert kw >= 0
            _WGRAD_KINDS.add(kw)
            mt = "%s wgrad mode %s: " % (tag, mode)

            def wgrad(T, acc):
                ws = ops._scratch(hplib.call("hpvg_conv_bwd_weight_ws_bytes", B, Ci, Co, T_, H, W, KT), T["dy"].device)
                hplib.call("hpvg_conv_bwd_weight_f32", p(T["dy"]), p(T["x"]), None, None, 0, p(T["dw"]), acc, *ws, B, Ci, Co, T_, H, W,
                           KT, hplib.stream())

            def wgrad_bias(T):
                ws = ops._scratch(hplib.call("hpvg_conv_bwd_weight_ws_bytes", B, Ci, Co, T_, H, W, KT), T["dy"].device)
                hplib.call("hpvg_conv_bwd_weight_bias_f32", p(T["dy"]), p(T["x"]), p(T["dw"]), 1, p(T["db"]), 1, *ws, B, Ci, Co, T_, H,
                           W, KT, hplib.stream())

            r = all_equal("a", sweep("a", mt + "overwrite", {"dy": dy, "x": x}, {"dw": (wsh, f32, None)}, lambda T: wgrad(T, 0)),
                          mt + "overwrite")
            check("a", r["dw"], G["dw"], G["dwA"], mt + "weight gradient", "wgrad", kw, names=wn)
            r = all_equal("a", sweep("a", mt + "into", {"dy": dy, "x": x}, {"dw": (wsh, f32, G["base"])}, lambda T: wgrad(T, 1)),
                          mt + "into")
            check("a", r["dw"], G["base64"] + G["dw"], G["base64"].abs().float() + G["dwA"], mt + "weight gradient, accumulate",
                  "wgrad.acc", kw, names=wn)
            acc = r["dw"]
            if fuses == 1:
                r = all_equal("a", sweep("a", mt + "weight+bias", {"dy": dy, "x": x},
                                         {"dw": (wsh, f32, G["base"]), "db": ((Co,), f32, G["bbase"])}, wgrad_bias), mt + "weight+bias")
                check("a", r["dw"], G["base64"] + G["dw"], G["base64"].abs().float() + G["dwA"], mt + "fused weight gradient",
                      "wgrad.fused", kw, names=wn)
                check("a", r["db"], G["bbase64"] + G["db"], G["bbase64"].abs().float() + G["dbA"], mt + "fused bias gradient",
                      "bias.fused", kw)
                assert torch.equal(r["dw"], acc), mt + "the fused launch's weight gradient differs from the plain launch's"
            else:
                assert hplib.load().hpvg_conv_bwd_weight_bias_f32(p(dy), p(x), p(G["base"].clone()), 1, p(G["bbase"].clone()), 1, None, 0,
                                                                  B, Ci, Co, T_, H, W, KT, hplib.stream()) != 0

    # the bias gradient of the layers that do not fuse it: the channel sum (the vector width follows dy's start; section (b)
    # walks the widths, here the default launch of this shape and its bit-equality within one width)
    def csum(T, acc):
        ws = ops._scratch(hplib.call("hpvg_channel_sum_ws_bytes", Co), T["dy"].device)
        hplib.call("hpvg_channel_sum_f32", p(T["dy"]), p(T["out"]), acc, *ws, B, Co, S, hplib.stream())

    done = sweep("a", tag + " channel sum", {"dy": dy}, {"out": ((Co,), f32, None)}, lambda T: csum(T, 0))
    _same_width_equal("a", done, lambda T: lib.hpvg_vec_width_at(p(T["dy"]), S), tag + " channel sum")
    for label, T, res in done:
        check("a", res["out"], G["db"], G["dbA"], tag + " channel sum [%s]" % label, "bias.sum", "V=%d" % lib.hpvg_vec_width_at(p(T["dy"]), S))
    _RAN["conv"].add(_conv_id((B, layer, sp)))


def _same_width_equal(sec, done, width_of, what):
    """Launches of one case that get the same vector width are equal bit for bit; returns {label: V}."""
    first, widths = {}, {}
    for label, T, res in done:
        V = int(width_of(T))
        assert V in (1, 2, 4), (what, label, V)
        widths[label] = V
        if V not in first:
            first[V] = (label, res)
            continue
        for n, t in first[V][1].items():
            assert torch.equal(res[n], t), "%s [%s]: %s differs from the [%s] launch of the same width V = %d" % (
                what, label, n, first[V][0], V)
        _COUNT[sec]["bit"] += 1
    return widths


def test_conv_two_axis_part_tiles_full_size(ops, hplib, lib):
    """video level 6, (7, 72, 129), 64 -> 64, B = 2: the persistent two-axis kernel runs its leftover round as part tiles
    (hpvg_conv_w2_split reports the cut).  Forward and backward-data with x at offset 0 and 2: equal bits, guards intact; no
    float64 reference (tests/test_conv_launches.py has it at offset 0)."""
    B, C, sp = 2, 64, (7, 72, 129)
    T_, H, W, KT = R.kernel_view(sp)
    out4 = (ctypes.c_int * 4)()
    assert lib.hpvg_conv_w2_split(B, C, C, T_, H, W, KT, out4) == 0
    assert out4[1] > 0 and out4[2] in (2, 4) and out4[3] > 0, list(out4)
    assert lib.hpvg_conv_fwd_kernel_kind(B, C, C, T_, H, W, KT) == 2
    _FWD_KINDS.add(2)
    g = _gen("w2", sp)
    x = _randn(g, B, C, *sp)
    w = _randn(g, C, C, 3, 3, 3) / (C * 27) ** 0.5
    shape = tuple(x.shape)
    cfgs = [("base", {}), ("x@2", {"x": 2})]
    for flip, name in ((False, "forward"), (True, "backward-data")):
        done = sweep("a", "two-axis part tiles, " + name, {"x": x, "w": w}, {"y": (shape, torch.float32, None)},
                     lambda T: _conv_launch(ops, hplib, T, (B, T_, H, W, KT), C, C, flip), configs=cfgs)
        all_equal("a", done, "two-axis part tiles, " + name)
    ops.weights_changed()


# ================================================================================================ (b) BatchNorm, channel sum
BN_SHAPES = [(2, 6, 8), (3, 5, 6), (3, 5, 7)]       # S = 96 = 0, 90 = 2, 105 = 1 (mod 4)
BN_CASES = [(sp, B, groups) for sp in BN_SHAPES for B, groups in E.BN_BATCHES]


def _bn_inputs(sp, B):
    g = _gen("bn", sp, B)
    C = E.BN_C
    one = (1, C) + (1,) * len(sp)
    r = _randn(g, B, C, *sp) * (0.5 + torch.rand(one, generator=g, device=DEV)) + (torch.rand(one, generator=g, device=DEV) * 2 - 1)
    return dict(r=r, dh=_randn(g, B, C, *sp), G=_randn(g, B, C, *sp), gamma=1 + 0.3 * _randn(g, C), beta=0.3 * _randn(g, C),
                rm=0.1 * _randn(g, C), rv=1 + 0.2 * torch.rand(C, generator=g, device=DEV), base_g=_randn(g, C), base_b=_randn(g, C))


def _note_width(S, widths):
    if S % 4 == 0:
        _V_BY_POINTER.update(widths.values())


def _stat_ptrs(hplib, st):
    return [hplib.ptr(st[j]) for j in range(4)]


@pytest.mark.parametrize("sp,B,groups", BN_CASES, ids=["%s-B%d-g%d" % ("x".join(map(str, c[0])), c[1], c[2]) for c in BN_CASES])
def test_bn_launches_at_every_offset(ops, hplib, lib, sp, B, groups):
    C, S = E.BN_C, E.spatial(sp)
    L = _bn_inputs(sp, B)
    shape = tuple(L["r"].shape)
    f32 = torch.float32
    p = hplib.ptr
    tag = "%s B=%d groups=%d: " % (tuple(sp), B, groups)
    mom, eps = E.BN_MOMENTUM, E.BN_EPS
    assert E.bn_plan_of(lib, B, S, groups)[0] == 1      # the fused path; the three-launch path has its own test below
    par = {"gamma": L["gamma"], "beta": L["beta"]}

    def gkey(V):
        return "V=%d%s" % (V, " g2" if groups == 2 else "")

    # ---- hpvg_bn_train_fwd_f32
    def fwd(T):
        ws = ops._scratch(hplib.call("hpvg_bn_ws_bytes", C * groups), T["r"].device)
        hplib.call("hpvg_bn_train_fwd_f32", p(T["r"]), p(T["gamma"]), p(T["beta"]), p(T["rm"]), p(T["rv"]), mom, eps,
                   *_stat_ptrs(hplib, T["stats"][0]), p(T["y"]), 1, groups, *ws, B, C, S, hplib.stream())

    done = sweep("b", tag + "bn_train_fwd", dict(r=L["r"], **par),
                 {"y": (shape, f32, None), "stats": ((groups, 4, C), f32, None), "rm": ((C,), f32, L["rm"]), "rv": ((C,), f32, L["rv"])},
                 fwd, vary=["r", "y"])
    widths = _same_width_equal("b", done, lambda T: lib.hpvg_bn_vec_width_at(p(T["r"]), B, C, S, groups), tag + "bn_train_fwd")
    _note_width(S, widths)
    ref = E.bn_fwd64(L["r"], L["gamma"], L["beta"], L["rm"], L["rv"], groups=groups, lrelu=True)
    for label, T, res in done:
        k, t = gkey(widths[label]), tag + "bn_train_fwd [%s] " % label
        check("b", res["y"], *ref["h"], t + "h", "bn.fwd.lrelu", k)
        for j, name in enumerate(("mean", "invstd", "scale", "shift")):
            check("b", res["stats"][:, j], *ref[name], t + name, "bn.stat", k, tau=E.TAU_STAT)
        check("b", res["rm"], *ref["rm"], t + "running_mean", "bn.running", k, tau=E.TAU_STAT)
        check("b", res["rv"], *ref["rv"], t + "running_var", "bn.running", k, tau=E.TAU_STAT)
    stats = done[0][2]["stats"].clone()

    # ---- hpvg_bn_act_bwd_f32 (fresh and accumulate form)
    def bwd(T, acc):
        ws = ops._scratch(hplib.call("hpvg_bn_ws_bytes", C * groups), T["r"].device)
        hplib.call("hpvg_bn_act_bwd_f32", p(T["dh"]), p(T["r"]), *_stat_ptrs(hplib, T["stats"][0]), 1, groups, p(T["dr"]), p(T["dgamma"]),
                   p(T["dbeta"]), acc, *ws, B, C, S, hplib.stream())

    def bwd_width(T):
        return min(lib.hpvg_bn_vec_width_at(p(T["dh"]), B, C, S, groups), lib.hpvg_bn_vec_width_at(p(T["r"]), B, C, S, groups))

    for acc, bg, bb in ((0, None, None), (1, L["base_g"], L["base_b"])):
        done = sweep("b", tag + "bn_act_bwd acc=%d" % acc, dict(dh=L["dh"], r=L["r"], stats=stats),
                     {"dr": (shape, f32, None), "dgamma": ((C,), f32, bg), "dbeta": ((C,), f32, bb)}, lambda T: bwd(T, acc),
                     vary=["dh", "r", "dr"])
        widths = _same_width_equal("b", done, bwd_width, tag + "bn_act_bwd")
        _note_width(S, widths)
        bref = E.bn_bwd64(L["dh"], L["r"], stats, groups=groups, lrelu=True, base_gamma=bg, base_beta=bb)
        for label, T, res in done:
            k, t = gkey(widths[label]), tag + "bn_act_bwd acc=%d [%s] " % (acc, label)
            check("b", res["dr"], *bref["dr"], t + "dr", "bn.bwd.lrelu", k)
            check("b", res["dgamma"], *bref["dgamma"], t + "dgamma", "bn.dgamma" + (".slot" if acc else ""), k)
            check("b", res["dbeta"], *bref["dbeta"], t + "dbeta", "bn.dbeta" + (".slot" if acc else ""), k)
    _RAN["bn"].add((tuple(sp), B, groups))
    if groups != 1:
        return

    # ---- the entry points without a group count: the batch is one group
    ref1 = ref
    stats1 = stats

    # hpvg_bn_train_stats_f32
    def stats_only(T):
        ws = ops._scratch(hplib.call("hpvg_bn_ws_bytes", C), T["r"].device)
        hplib.call("hpvg_bn_train_stats_f32", p(T["r"]), p(T["gamma"]), p(T["beta"]), p(T["rm"]), p(T["rv"]), mom, eps,
                   *_stat_ptrs(hplib, T["stats"][0]), *ws, B, C, S, hplib.stream())

    # hpvg_bn_sums_f32 + hpvg_bn_finalize_f32 (the batch-split form with one rank)
    def sums_finalize(T):
        ws = ops._scratch(hplib.call("hpvg_bn_ws_bytes", C), T["r"].device)
        sums = torch.full((C, 2), float("nan"), dtype=torch.float64, device=DEV)
        hplib.call("hpvg_bn_sums_f32", p(T["r"]), p(sums), *ws, B, C, S, hplib.stream())
        hplib.call("hpvg_bn_finalize_f32", p(sums), float(B) * float(S), p(T["gamma"]), p(T["beta"]), p(T["rm"]), p(T["rv"]), mom, eps,
                   *_stat_ptrs(hplib, T["stats"][0]), C, hplib.stream())
        return {"sums": sums}

    for name, fn in (("bn_train_stats", stats_only), ("bn_sums+finalize", sums_finalize)):
        done = sweep("b", tag + name, dict(r=L["r"], **par),
                     {"stats": ((1, 4, C), f32, None), "rm": ((C,), f32, L["rm"]), "rv": ((C,), f32, L["rv"])}, fn, vary=["r"])
        widths = _same_width_equal("b", done, lambda T: lib.hpvg_vec_width_at(p(T["r"]), S), tag + name)
        _note_width(S, widths)
        for label, T, res in done:
            k, t = gkey(widths[label]), tag + name + " [%s] " % label
            for j, sname in enumerate(("mean", "invstd", "scale", "shift")):
                check("b", res["stats"][:, j], *ref1[sname], t + sname, name + ".stat", k, tau=E.TAU_STAT)
            check("b", res["rm"], *ref1["rm"], t + "running_mean", name + ".running", k, tau=E.TAU_STAT)
            check("b", res["rv"], *ref1["rv"], t + "running_var", name + ".running", k, tau=E.TAU_STAT)

    # the _sums / _apply pair of the backward
    def bwd_pair(T):
        ws = ops._scratch(hplib.call("hpvg_bn_ws_bytes", C), T["r"].device)
        sums = torch.full((C, 2), float("nan"), dtype=torch.float64, device=DEV)
        st = _stat_ptrs(hplib, T["stats"][0])
        hplib.call("hpvg_bn_act_bwd_sums_f32", p(T["dh"]), p(T["r"]), *st, 1, p(sums), *ws, B, C, S, hplib.stream())
        gsum = sums.to(torch.float32).contiguous()
        hplib.call("hpvg_bn_act_bwd_apply_f32", p(T["dh"]), p(T["r"]), *st, 1, p(gsum), float(1.0 / (float(B) * float(S))), p(T["dr"]),
                   B, C, S, hplib.stream())
        return {"dbeta": sums[:, 0].contiguous(), "dgamma": sums[:, 1].contiguous()}

    done = sweep("b", tag + "bn_act_bwd_sums+apply", dict(dh=L["dh"], r=L["r"], stats=stats1), {"dr": (shape, f32, None)}, bwd_pair,
                 vary=["dh", "r", "dr"])
    widths = _same_width_equal("b", done, lambda T: min(lib.hpvg_vec_width_at(p(T["dh"]), S), lib.hpvg_vec_width_at(p(T["r"]), S)),
                               tag + "bn_act_bwd_sums+apply")
    _note_width(S, widths)
    bref = E.bn_bwd64(L["dh"], L["r"], stats1, groups=1, lrelu=True)
    for label, T, res in done:
        k, t = gkey(widths[label]), tag + "bn_act_bwd_sums+apply [%s] " % label
        check("b", res["dr"], *bref["dr"], t + "dr", "sync.bwd.lrelu", k)
        check("b", res["dgamma"], *bref["dgamma"], t + "dgamma", "sync.dgamma", k)
        check("b", res["dbeta"], *bref["dbeta"], t + "dbeta", "sync.dbeta", k)

    # ---- hpvg_bn_act_bwd2_f32
    def bwd2(T):
        ws = ops._scratch(hplib.call("hpvg_bn_bwd2_ws_bytes", C), T["r"].device)
        hplib.call("hpvg_bn_act_bwd2_f32", p(T["dh"]), p(T["G"]), p(T["r"]), *_stat_ptrs(hplib, T["stats"][0]), 1, p(T["g_dh"]),
                   p(T["g_r"]), p(T["g_gamma"]), 0, *ws, B, C, S, hplib.stream())

    done = sweep("b", tag + "bn_act_bwd2", dict(dh=L["dh"], G=L["G"], r=L["r"], stats=stats1),
                 {"g_dh": (shape, f32, None), "g_r": (shape, f32, None), "g_gamma": ((C,), f32, None)}, bwd2,
                 vary=["dh", "G", "r", "g_dh", "g_r"])
    widths = _same_width_equal("b", done, lambda T: min(lib.hpvg_vec_width_at(p(T[n]), S) for n in ("dh", "G", "r")), tag + "bn_act_bwd2")
    _note_width(S, widths)
    r2 = E.bn_bwd2_64(L["dh"], L["G"], L["r"], stats1, lrelu=True)
    for label, T, res in done:
        k, t = gkey(widths[label]), tag + "bn_act_bwd2 [%s] " % label
        for n in ("g_dh", "g_r", "g_gamma"):
            check("b", res[n], *r2[n], t + n, "bn2." + n, k)


# the channel sum in its one-pass form (a single split: B * S <= 2048) at the BatchNorm shapes, and in its two-pass form at the
# smallest shapes of the same residues of S above that
CSUM_CASES = [(sp, 2, 1) for sp in BN_SHAPES] + [((9, 16, 16), 1, 2), ((3, 27, 34), 1, 2), ((3, 27, 35), 1, 2)]


@pytest.mark.parametrize("sp,B,passes", CSUM_CASES, ids=["%s-B%d-%dpass" % ("x".join(map(str, c[0])), c[1], c[2]) for c in CSUM_CASES])
def test_channel_sum_at_every_offset(ops, hplib, lib, sp, B, passes):
    C, S = E.BN_C, E.spatial(sp)
    assert ((B * S + 2047) // 2048 > 1) == (passes == 2)      # hpvg_channel_sum_f32's split rule (C = 64 wants 16)
    g = _gen("csum", sp, B)
    x, base = _randn(g, B, C, *sp), _randn(g, C)
    p = hplib.ptr
    ref, A = R.bias_sum64_on(x)
    tag = "channel sum %s B=%d (%d-pass): " % (tuple(sp), B, passes)
    for acc, init in ((0, None), (1, base)):
        def run(T):
            ws = ops._scratch(hplib.call("hpvg_channel_sum_ws_bytes", C), T["x"].device)
            hplib.call("hpvg_channel_sum_f32", p(T["x"]), p(T["out"]), acc, *ws, B, C, S, hplib.stream())

        done = sweep("b", tag + "acc=%d" % acc, {"x": x}, {"out": ((C,), torch.float32, init)}, run)
        widths = _same_width_equal("b", done, lambda T: lib.hpvg_vec_width_at(p(T["x"]), S), tag)
        _note_width(S, widths)
        assert set(widths.values()) == ({4, 2, 1} if S % 4 == 0 else {2, 1} if S % 2 == 0 else {1})
        r64, a64 = (ref, A) if init is None else (base.double() + ref, base.abs() + A)
        for label, T, res in done:
            check("b", res["out"], r64, a64, tag + "[%s]" % label, "csum.%dpass%s" % (passes, ".acc" if acc else ""), "V=%d" % widths[label])


def test_bn_three_launch_path_at_offset(ops, hplib, lib):
    """Above HPVG_BN_FUSE_MAX (2 * 64 * S > 2^25) the forward and the backward run three launches per group with their own
    per-group pointer arithmetic.  S = 2^18 + 4, the smallest multiple of 4 above the bound, as (2, 2, 65537); r at offset 2, so
    that the pointer picks V = 2 on an S % 4 == 0 shape; float64 reference on the device."""
    B, C, sp = 2, E.BN_C, (2, 2, 65537)
    S = E.spatial(sp)
    assert S % 4 == 0 and S == (1 << 18) + 4 and B * C * S > 1 << 25 and B * C * (S - 4) <= 1 << 25
    assert E.bn_plan_of(lib, B, S, 1) == (0, 16, 4)
    L = _bn_inputs(sp, B)
    shape = tuple(L["r"].shape)
    f32 = torch.float32
    p = hplib.ptr
    cfgs = [("base", {}), ("r@2", {"r": 2})]

    def fwd(T):
        ws = ops._scratch(hplib.call("hpvg_bn_ws_bytes", C), T["r"].device)
        hplib.call("hpvg_bn_train_fwd_f32", p(T["r"]), p(T["gamma"]), p(T["beta"]), p(T["rm"]), p(T["rv"]), E.BN_MOMENTUM, E.BN_EPS,
                   *_stat_ptrs(hplib, T["stats"][0]), p(T["y"]), 1, 1, *ws, B, C, S, hplib.stream())

    done = sweep("b", "three-launch bn_train_fwd", dict(r=L["r"], gamma=L["gamma"], beta=L["beta"]),
                 {"y": (shape, f32, None), "stats": ((1, 4, C), f32, None), "rm": ((C,), f32, L["rm"]), "rv": ((C,), f32, L["rv"])},
                 fwd, configs=cfgs)
    widths = _same_width_equal("b", done, lambda T: lib.hpvg_vec_width_at(p(T["r"]), S), "three-launch bn_train_fwd")
    assert widths == {"base": 4, "r@2": 2}
    _V_BY_POINTER.update(widths.values())
    ref = E.bn_fwd64(L["r"], L["gamma"], L["beta"], L["rm"], L["rv"], groups=1, lrelu=True)
    for label, T, res in done:
        k = "3-launch V=%d" % widths[label]
        check("b", res["y"], *ref["h"], "three-launch h [%s]" % label, "bn.fwd.lrelu", k)
        for j, name in enumerate(("mean", "invstd", "scale", "shift")):
            check("b", res["stats"][:, j], *ref[name], "three-launch %s [%s]" % (name, label), "bn.stat", k, tau=E.TAU_STAT)
        check("b", res["rm"], *ref["rm"], "three-launch running_mean [%s]" % label, "bn.running", k, tau=E.TAU_STAT)
        check("b", res["rv"], *ref["rv"], "three-launch running_var [%s]" % label, "bn.running", k, tau=E.TAU_STAT)
    stats = done[0][2]["stats"].clone()
    del ref, done

    def bwd(T):
        ws = ops._scratch(hplib.call("hpvg_bn_ws_bytes", C), T["r"].device)
        hplib.call("hpvg_bn_act_bwd_f32", p(T["dh"]), p(T["r"]), *_stat_ptrs(hplib, T["stats"][0]), 1, 1, p(T["dr"]), p(T["dgamma"]),
                   p(T["dbeta"]), 0, *ws, B, C, S, hplib.stream())

    done = sweep("b", "three-launch bn_act_bwd", dict(dh=L["dh"], r=L["r"], stats=stats),
                 {"dr": (shape, f32, None), "dgamma": ((C,), f32, None), "dbeta": ((C,), f32, None)}, bwd, configs=cfgs)
    widths = _same_width_equal("b", done, lambda T: min(lib.hpvg_vec_width_at(p(T["dh"]), S), lib.hpvg_vec_width_at(p(T["r"]), S)),
                               "three-launch bn_act_bwd")
    assert widths == {"base": 4, "r@2": 2}
    bref = E.bn_bwd64(L["dh"], L["r"], stats, groups=1, lrelu=True)
    for label, T, res in done:
        k = "3-launch V=%d" % widths[label]
        check("b", res["dr"], *bref["dr"], "three-launch dr [%s]" % label, "bn.bwd.lrelu", k)
        check("b", res["dgamma"], *bref["dgamma"], "three-launch dgamma [%s]" % label, "bn.dgamma", k)
        check("b", res["dbeta"], *bref["dbeta"], "three-launch dbeta [%s]" % label, "bn.dbeta", k)
    del bref, done, L
    torch.cuda.empty_cache()


# ================================================================================================ (c) pointwise, losses, ...
EW_SHAPES = [((2, 3, 3, 5, 7), (4, 7, 9)), ((2, 3, 5, 7), (7, 9))]     # input, resize target
EW_IDS = ["3d", "2d"]


def _leaf(t):
    return t.detach().requires_grad_(True)


@pytest.mark.parametrize("shape,size", EW_SHAPES, ids=EW_IDS)
def test_pointwise_and_losses_through_ops_at_every_offset(ops, hplib, lib, shape, size):
    """TanhRes, Add, LReLUMaskMul, Reparam, KL, MSE, MeanScaled, GradPenalty forward and backward, lerp, sqsum and
    concat_batch through ops with every input in turn at offset 1, 2, 3: bit-equal to the base, scalars included."""
    g = _gen("ew", shape)
    a, b, c, dy = (_randn(g, *shape) for _ in range(4))
    lv = 0.5 * _randn(g, *shape)
    gr = 0.7 * _randn(g, *shape)
    gr[(1, slice(None)) + (0,) * (len(shape) - 2)] = 0       # one voxel of zero norm
    gout = torch.tensor(0.83, device=DEV)
    alpha = torch.tensor([0.37], device=DEV)
    key = "%dd" % (len(shape) - 2)
    lam = 0.1
    tag = "%s: " % (shape,)

    def run_tanh(T):
        x = _leaf(T["x"])
        res = _leaf(T["res"]) if T.get("res") is not None else None
        y = ops.TanhRes.apply(x, res)
        grads = torch.autograd.grad(y, [x] + ([res] if res is not None else []), T["dy"])
        return dict(y=y.detach(), dx=grads[0])

    r = all_equal("c", sweep("c", tag + "TanhRes", {"x": a, "res": b, "dy": dy}, {}, run_tanh), tag + "TanhRes")
    assert_close(r["y"], torch.tanh(a.double() + b.double()), RTOL, "tanh")
    assert_close(r["dx"], dy.double() * (1 - torch.tanh(a.double() + b.double()) ** 2), RTOL, "tanh.bwd")
    all_equal("c", sweep("c", tag + "TanhRes without res", {"x": a, "res": None, "dy": dy}, {}, run_tanh), tag + "TanhRes without res")

    r = all_equal("c", sweep("c", tag + "Add", {"a": a, "b": b}, {}, lambda T: {"out": ops.Add.apply(T["a"], T["b"])}), tag + "Add")
    assert torch.equal(r["out"], a + b)
    r = all_equal("c", sweep("c", tag + "LReLUMaskMul", {"dy": dy, "h": a}, {}, lambda T: {"out": ops.LReLUMaskMul.apply(T["dy"], T["h"])}),
                  tag + "LReLUMaskMul")
    assert_close(r["out"], dy.double() * torch.where(a > 0, 1.0, 0.2).double(), 1e-6, "lrelu_mask_mul")

    def run_reparam(T):
        mu, l = _leaf(T["mu"]), _leaf(T["lv"])
        z = ops.Reparam.apply(mu, l, T["eps"])
        dmu, dl = torch.autograd.grad(z, [mu, l], T["dz"])
        return dict(z=z.detach(), dmu=dmu, dlv=dl)

    r = all_equal("c", sweep("c", tag + "Reparam", {"mu": a, "lv": lv, "eps": c, "dz": dy}, {}, run_reparam), tag + "Reparam")
    assert_close(r["z"], c.double() * torch.exp(0.5 * lv.double()) + a.double(), RTOL, "reparam")
    assert_close(r["dlv"], dy.double() * c.double() * 0.5 * torch.exp(0.5 * lv.double()), RTOL, "reparam.bwd")

    def run_kl(T):
        mu, l = _leaf(T["mu"]), _leaf(T["lv"])
        k = ops.KL.apply(mu, l)
        dmu, dl = torch.autograd.grad(k, [mu, l], gout)
        return dict(kl=k.detach().reshape(1), dmu=dmu, dlv=dl)

    r = all_equal("c", sweep("c", tag + "KL", {"mu": a, "lv": lv}, {}, run_kl), tag + "KL")
    check_scalar("c", r["kl"], *E.kl64(a, lv), tag + "KL", "kl.fwd", key)
    (dm, dmA), (dl_, dlA) = E.kl_bwd64(float(gout), a, lv)
    check("c", r["dmu"], dm, dmA, tag + "KL dmu", "kl.bwd", key)
    check("c", r["dlv"], dl_, dlA, tag + "KL dlogvar", "kl.bwd", key)

    def run_mse(T):
        al, bl = _leaf(T["a"]), _leaf(T["b"])
        m = ops.MSE.apply(al, bl)
        da, db = torch.autograd.grad(m, [al, bl], gout)
        return dict(mse=m.detach().reshape(1), da=da, db=db)

    r = all_equal("c", sweep("c", tag + "MSE", {"a": a, "b": b}, {}, run_mse), tag + "MSE")
    check_scalar("c", r["mse"], *E.mse64(a, b), tag + "MSE", "mse.fwd", key)
    check("c", r["da"], *E.mse_bwd64(float(gout), a, b), tag + "MSE da", "mse.bwd", key)
    check("c", r["db"], *E.mse_bwd64(float(gout), b, a), tag + "MSE db", "mse.bwd", key)

    def run_ms(T):
        x = _leaf(T["x"])
        m = ops.MeanScaled.apply(x, -1.0)
        (dx,) = torch.autograd.grad(m, [x], gout)
        return dict(ms=m.detach().reshape(1), dx=dx)

    r = all_equal("c", sweep("c", tag + "MeanScaled", {"x": a}, {}, run_ms), tag + "MeanScaled")
    check_scalar("c", r["ms"], *E.mean_scaled64(a, -1.0), tag + "MeanScaled", "meanscaled.fwd", key)
    coef = torch.full_like(a, -1.0 / a.numel(), dtype=torch.float64) * float(gout)
    check("c", r["dx"], coef, coef.abs(), tag + "MeanScaled backward", "meanscaled.bwd", key)

    def run_gp(T):
        gl = _leaf(T["g"])
        P = ops.GradPenalty.apply(gl, lam)
        (dg,) = torch.autograd.grad(P, [gl], gout)
        return dict(gp=P.detach().reshape(1), dg=dg)

    r = all_equal("c", sweep("c", tag + "GradPenalty", {"g": gr}, {}, run_gp), tag + "GradPenalty")
    check_scalar("c", r["gp"], *E.gp64(gr, lam), tag + "gradient penalty", "gp.fwd", key)
    check("c", r["dg"], *E.gp_bwd64(float(gout), gr, lam), tag + "gradient penalty backward", "gp.bwd", key)

    r = all_equal("c", sweep("c", tag + "lerp", {"a": a, "b": b, "alpha": alpha}, {}, lambda T: {"out": ops.lerp(T["a"], T["b"], T["alpha"])}),
                  tag + "lerp")
    assert_close(r["out"], 0.37 * a.double() + (1 - 0.37) * b.double(), 1e-6, "lerp")
    r = all_equal("c", sweep("c", tag + "sqsum", {"x": a}, {}, lambda T: {"sq": ops.sqsum(T["x"].view(-1))}), tag + "sqsum")
    check_scalar("c", r["sq"], *E.sqsum64(a), tag + "sqsum", "sqsum", key)
    r = all_equal("c", sweep("c", tag + "concat_batch", {"a": a, "b": b[:1].contiguous()}, {},
                             lambda T: {"out": ops.concat_batch([T["a"], 1, T["b"]])}), tag + "concat_batch")
    assert torch.equal(r["out"], torch.cat([a, torch.zeros_like(a[:1]), b[:1]]))


# the kernels behind the Functions above, called directly so that the OUTPUT pointer is ours: name, inputs, outputs
def _pointwise_table(n):
    L = ctypes.c_long(n)
    return [
        ("hpvg_tanh_fwd_f32", ["x", "res"], ["y"], lambda p, T, s: (p(T["x"]), p(T["res"]), p(T["y"]), L, s)),
        ("hpvg_tanh_bwd_f32", ["dy", "x"], ["y"], lambda p, T, s: (p(T["dy"]), p(T["x"]), p(T["y"]), L, s)),
        ("hpvg_add_f32", ["x", "res"], ["y"], lambda p, T, s: (p(T["x"]), p(T["res"]), p(T["y"]), L, s)),
        ("hpvg_lrelu_mask_mul_f32", ["dy", "x"], ["y"], lambda p, T, s: (p(T["dy"]), p(T["x"]), p(T["y"]), L, s)),
        ("hpvg_reparam_fwd_f32", ["x", "lv", "res"], ["y"], lambda p, T, s: (p(T["x"]), p(T["lv"]), p(T["res"]), p(T["y"]), L, s)),
        ("hpvg_reparam_bwd_f32", ["dy", "lv", "res"], ["y"], lambda p, T, s: (p(T["dy"]), p(T["lv"]), p(T["res"]), p(T["y"]), L, s)),
        ("hpvg_kl_bwd_f32", ["gout", "x", "lv"], ["y", "y2"], lambda p, T, s: (p(T["gout"]), p(T["x"]), p(T["lv"]), p(T["y"]), p(T["y2"]), L, s)),
        ("hpvg_mse_bwd_f32", ["gout", "x", "res"], ["y"], lambda p, T, s: (p(T["gout"]), p(T["x"]), p(T["res"]), p(T["y"]), L, s)),
        ("hpvg_fill_scaled_f32", ["gout"], ["y"], lambda p, T, s: (p(T["gout"]), 0.25, p(T["y"]), L, s)),
        ("hpvg_lerp_f32", ["x", "res", "gout"], ["y"], lambda p, T, s: (p(T["x"]), p(T["res"]), p(T["gout"]), p(T["y"]), L, s)),
        ("hpvg_copy_f32", ["x"], ["y"], lambda p, T, s: (p(T["x"]), p(T["y"]), L, s)),
        ("hpvg_copy_f32 (zero fill)", [], ["y"], lambda p, T, s: (None, p(T["y"]), L, s)),
    ]


@pytest.mark.parametrize("shape,size", EW_SHAPES, ids=EW_IDS)
def test_pointwise_kernels_into_guarded_outputs(ops, hplib, lib, shape, size):
    """The same kernels through the C ABI with inputs AND outputs at every offset: outputs bit-equal to the base, their guards
    intact, every element stored; the gradient penalty's backward with its (B, C, S) arguments."""
    g = _gen("ewdirect", shape)
    n = 1
    for v in shape:
        n *= v
    pool = dict(x=_randn(g, *shape), res=_randn(g, *shape), dy=_randn(g, *shape), lv=0.5 * _randn(g, *shape),
                gout=torch.tensor([0.83], device=DEV))
    p = hplib.ptr
    for name, ins, outs, args in _pointwise_table(n):
        def run(T):
            hplib.call(name.split()[0], *args(p, T, hplib.stream()))

        r = all_equal("c", sweep("c", name, {k: pool[k] for k in ins}, {k: (shape, torch.float32, None) for k in outs}, run), name)
        if name == "hpvg_copy_f32":
            assert torch.equal(r["y"], pool["x"])
        elif name.endswith("(zero fill)"):
            assert not bool(r["y"].any())
    B, C = shape[0], shape[1]
    S = n // (B * C)

    def run_gp(T):
        ws = ops._reduce_ws(T["x"].device)
        hplib.call("hpvg_gp_fwd_f32", p(T["x"]), p(T["P"]), 0.1, *ws, B, C, S, hplib.stream())
        hplib.call("hpvg_gp_bwd_f32", p(T["gout"]), p(T["x"]), p(T["y"]), 0.1, B, C, S, hplib.stream())

    all_equal("c", sweep("c", "hpvg_gp_fwd/bwd_f32", {"x": pool["x"], "gout": pool["gout"]},
                         {"y": (shape, torch.float32, None), "P": ((1,), torch.float32, None)}, run_gp), "hpvg_gp_fwd/bwd_f32")


@pytest.mark.parametrize("shape,size", EW_SHAPES, ids=EW_IDS)
def test_resize_at_every_offset(ops, hplib, lib, shape, size):
    """UpsampleAC with and without a noise tensor and UpsampleACNoise, forward and backward, through ops with every input at
    every offset, and the three kernels through the C ABI into guarded outputs."""
    g = _gen("resize", shape)
    B, C = shape[0], shape[1]
    oshape = (B, C) + tuple(size)
    x, noise, dy, dy2 = _randn(g, *shape), _randn(g, *oshape), _randn(g, *oshape), _randn(g, *oshape)
    amp, first_noisy, call0 = 0.37, 1, 4242
    st = ops._rng(torch.device(DEV))
    key = "%dd" % len(size)
    tag = "resize %s -> %s: " % (shape, tuple(size))
    p = hplib.ptr

    def run_ops(T):
        xl = _leaf(T["x"])
        y = ops.UpsampleAC.apply(xl, tuple(size), None, 0.0)
        (dx,) = torch.autograd.grad(y, [xl], T["dy"])
        y2, yn = ops.UpsampleAC.apply(xl, tuple(size), T["noise"], amp)
        (dx2,) = torch.autograd.grad([y2, yn], [xl], [T["dy"], T["dy2"]])
        st.call = call0
        y3, yn3 = ops.UpsampleACNoise.apply(xl, tuple(size), amp, first_noisy)
        (dx3,) = torch.autograd.grad([y3, yn3], [xl], [T["dy"], T["dy2"]])
        return dict(y=y.detach(), dx=dx, y2=y2.detach(), yn=yn.detach(), dx2=dx2, y3=y3.detach(), yn3=yn3.detach(), dx3=dx3)

    r = all_equal("c", sweep("c", tag + "through ops", {"x": x, "noise": noise, "dy": dy, "dy2": dy2}, {}, run_ops), tag + "through ops")
    nz = torch.empty(oshape, device=DEV)
    hplib.call("hpvg_normal_f32", p(nz), ctypes.c_long(nz.numel()), ops._seed(), ctypes.c_uint(call0), p(st.iter_dev), hplib.stream())
    yref, yA, ynref, ynA = E.resize64(x, size, noise, amp)
    check("c", r["y"], yref, yA, tag + "y", "resize.fwd", key)
    assert torch.equal(r["y2"], r["y"]), tag + "y differs between the launches with and without a noise tensor"
    check("c", r["y3"], yref, yA, tag + "y of the noise-generating kernel", "resize.fwd.noisegen", key)
    check("c", r["yn"], ynref, ynA, tag + "y + amp*noise", "resize.fwd.noise", key)
    _, _, yn3ref, yn3A = E.resize64(x, size, nz, amp)
    check("c", r["yn3"][first_noisy:], yn3ref[first_noisy:], yn3A[first_noisy:], tag + "y + amp*N(0,1)", "resize.fwd.noisegen", key)
    assert torch.equal(r["yn3"][:first_noisy], r["y3"][:first_noisy])
    check("c", r["dx"], *E.resize_bwd64(dy, shape[2:]), tag + "dx", "resize.bwd", key)
    check("c", r["dx2"], *E.resize_bwd64(dy, shape[2:], dy2), tag + "dx from dy + dy2", "resize.bwd.dy2", key)
    assert torch.equal(r["dx3"], r["dx2"])

    Ti, Hi, Wi = (shape[2:] if len(size) == 3 else (1,) + tuple(shape[2:]))
    To, Ho, Wo = (size if len(size) == 3 else (1,) + tuple(size))
    dims = (B * C, Ti, Hi, Wi, To, Ho, Wo)
    f32 = torch.float32

    def fwd(T):
        hplib.call("hpvg_upsample_linear_ac_f32", p(T["x"]), p(T["y"]), p(T.get("noise")), amp, p(T.get("yn")), *dims, hplib.stream())

    d = all_equal("c", sweep("c", tag + "kernel", {"x": x}, {"y": (oshape, f32, None)}, fwd), tag + "kernel")
    assert torch.equal(d["y"], r["y"])
    d = all_equal("c", sweep("c", tag + "kernel + noise", {"x": x, "noise": noise}, {"y": (oshape, f32, None), "yn": (oshape, f32, None)}, fwd),
                  tag + "kernel + noise")
    assert torch.equal(d["y"], r["y"]) and torch.equal(d["yn"], r["yn"])

    def fwd_noise(T):
        hplib.call("hpvg_upsample_linear_ac_noise_f32", p(T["x"]), p(T["y"]), p(T["yn"]), amp, dims[0], C, first_noisy, *dims[1:],
                   ops._seed(), ctypes.c_uint(call0), p(st.iter_dev), hplib.stream())

    d = all_equal("c", sweep("c", tag + "noise kernel", {"x": x}, {"y": (oshape, f32, None), "yn": (oshape, f32, None)}, fwd_noise),
                  tag + "noise kernel")
    assert torch.equal(d["y"], r["y3"]) and torch.equal(d["yn"], r["yn3"])

    def bwd(T):
        hplib.call("hpvg_upsample_linear_ac_bwd_f32", p(T["dy"]), p(T.get("dy2")), p(T["dx"]), *dims, hplib.stream())

    d = all_equal("c", sweep("c", tag + "backward kernel", {"dy": dy, "dy2": dy2}, {"dx": (shape, f32, None)}, bwd), tag + "backward kernel")
    assert torch.equal(d["dx"], r["dx2"])
    d = all_equal("c", sweep("c", tag + "backward kernel, dy alone", {"dy": dy}, {"dx": (shape, f32, None)}, bwd), tag + "backward kernel, dy alone")
    assert torch.equal(d["dx"], r["dx"])


@pytest.mark.parametrize("shape,size", EW_SHAPES, ids=EW_IDS)
def test_noise_into_offset_outputs(ops, hplib, lib, shape, size):
    """ops.normal_ and ops.uniform_ into an out_like whose numel is not a multiple of 4: the same draw at every offset, guards
    intact."""
    n = 1
    for v in shape:
        n *= v
    assert n % 4 != 0
    st = ops._rng(torch.device(DEV))
    for name, fn in (("normal_", ops.normal_), ("uniform_", ops.uniform_)):
        def run(T):
            st.call = 77
            fn(T["out"])

        r = all_equal("c", sweep("c", name, {}, {"out": (shape, torch.float32, None)}, run), name)
        if name == "uniform_":
            assert float(r["out"].min()) >= 0.0 and float(r["out"].max()) < 1.0
        else:
            assert abs(float(r["out"].mean())) < 0.3 and 0.7 < float(r["out"].std()) < 1.3   # 210 or 630 draws: > 4 sigma


@pytest.mark.parametrize("shape,size", EW_SHAPES, ids=EW_IDS)
def test_pad_and_crop_through_ops_at_every_offset(ops, hplib, lib, shape, size):
    g = _gen("pad", shape)
    x, gpad = _randn(g, *shape), None
    nd = len(shape) - 2
    tag = "%s: " % (shape,)

    def run(T):
        xl = _leaf(T["x"])
        y = ops.ZeroPad.apply(xl, 2)
        (dx,) = torch.autograd.grad(y, [xl], T["g"])
        c = ops.CropBorder.apply(T["x"], 1)
        return dict(pad=y.detach(), dx=dx, crop=c)

    gpad = _randn(g, *(shape[:2] + tuple(v + 4 for v in shape[2:])))
    r = all_equal("c", sweep("c", tag + "ZeroPad / CropBorder", {"x": x, "g": gpad}, {}, run), tag + "ZeroPad / CropBorder")
    assert torch.equal(r["pad"], F.pad(x, (2, 2) * nd))
    inner = (slice(None), slice(None)) + (slice(2, -2),) * nd
    assert torch.equal(r["dx"], gpad[inner])
    assert torch.equal(r["crop"], x[(slice(None), slice(None)) + (slice(1, -1),) * nd])


# BC = 4, 1, 3 planes of (1, 3, 5) padded by 1 to (3, 5, 7): n = 420, 105, 315 = 0, 1, 3 (mod 4)
@pytest.mark.parametrize("BC", [4, 1, 3])
def test_box_copy_store_forms(ops, hplib, lib, BC):
    """hpvg_box_copy_f32 with dst at offset 0 (16-byte stores) and 1, 2, 3 (element stores): equal bits, also for a tail of 1 or
    3 elements; pad and crop; src at every offset too."""
    g = _gen("box", BC)
    src = _randn(g, BC, 1, 3, 5)
    p = hplib.ptr
    n = BC * 105
    assert n % 4 == {4: 0, 1: 1, 3: 3}[BC]

    def pad(T):
        _BOX_FORMS.add("16-byte" if T["dst"].data_ptr() % 16 == 0 else "element")
        hplib.call("hpvg_box_copy_f32", p(T["src"]), p(T["dst"]), ctypes.c_long(BC), 1, 3, 5, 3, 5, 7, 1, 1, 1, hplib.stream())

    r = all_equal("c", sweep("c", "box_copy pad BC=%d" % BC, {"src": src}, {"dst": ((BC, 3, 5, 7), torch.float32, None)}, pad),
                  "box_copy pad BC=%d" % BC)
    assert torch.equal(r["dst"], F.pad(src, (1, 1, 1, 1, 1, 1)))
    big = r["dst"].clone()

    def crop(T):
        hplib.call("hpvg_box_copy_f32", p(T["src"]), p(T["dst"]), ctypes.c_long(BC), 3, 5, 7, 1, 3, 5, -1, -1, -1, hplib.stream())

    r = all_equal("c", sweep("c", "box_copy crop BC=%d" % BC, {"src": big}, {"dst": ((BC, 1, 3, 5), torch.float32, None)}, crop),
                  "box_copy crop BC=%d" % BC)
    assert torch.equal(r["dst"], src)
    _RAN["box"].add(BC)


@pytest.mark.parametrize("shape,size", EW_SHAPES, ids=EW_IDS)
def test_variant_kernels_at_every_offset(ops, hplib, lib, shape, size):
    """The kernels of csrc/variants.hip (Gate, GlobalAvgPool, CodeTimesMap, ReparamBern, KLBern) through the C ABI with every
    input and output in turn at offset 1, 2, 3: bit-equal to the base, guards intact, every element stored; the base against
    the float64 references of tests/variant_ref.py (S = 105 / 35: odd, so rows start at every residue)."""
    import variant_ref as V
    g = _gen("variants", shape)
    B, C = shape[0], shape[1]
    S = E.spatial(shape[2:])
    key = "%dd" % (len(shape) - 2)
    f32 = torch.float32
    p = hplib.ptr
    f, dout, dz = (_randn(g, B, C, S) for _ in range(3))
    logit, ext, zmap = 2 * _randn(g, B, S), _randn(g, B, S), _randn(g, B, S)
    code = _randn(g, B, C)
    x = torch.rand(B, S, generator=g, device=DEV) * 0.98 + 0.01
    eps = torch.rand(B, S, generator=g, device=DEV)
    gout = torch.tensor([0.83], device=DEV)
    L = ctypes.c_long(B * S)
    tag = "variants %s: " % (shape,)

    def launch(name, *args):
        hplib.call(name, *args, hplib.stream())

    r = all_equal("c", sweep("c", tag + "gate_fwd", {"f": f, "logit": logit}, {"out": ((B, C, S), f32, None), "bern": ((B, S), f32, None)},
                             lambda T: launch("hpvg_gate_fwd_f32", p(T["f"]), p(T["logit"]), p(T["out"]), p(T["bern"]), B, C, S)),
                  tag + "gate_fwd")
    ref = V.gate_fwd64(f, logit)
    check("c", r["out"], *ref["out"], tag + "gate out", "gate.out", key)
    check("c", r["bern"], *ref["bern"], tag + "gate bern", "gate.bern", key)
    bern = r["bern"].clone()
    for dname, d, e in (("both", dout, ext), ("dout", dout, None), ("dbern_ext", None, ext)):
        r = all_equal("c", sweep("c", tag + "gate_bwd " + dname, {"dout": d, "f": f, "bern": bern, "ext": e},
                                 {"df": ((B, C, S), f32, None), "dlogit": ((B, S), f32, None)},
                                 lambda T: launch("hpvg_gate_bwd_f32", p(T["dout"]), p(T["f"]), p(T["bern"]), p(T["ext"]), p(T["df"]),
                                                  p(T["dlogit"]), B, C, S)), tag + "gate_bwd " + dname)
        bref = V.gate_bwd64(d, f, bern, e)
        check("c", r["df"], *bref["df"], tag + "gate df " + dname, "gate.df", key)
        check("c", r["dlogit"], *bref["dlogit"], tag + "gate dlogit " + dname, "gate.dlogit", key)
    for wname, w, scale in (("pool", None, 1.0 / S), ("weighted", zmap, 1.0)):
        r = all_equal("c", sweep("c", tag + "rowsum " + wname, {"x": dz, "w": w}, {"out": ((B, C), f32, None)},
                                 lambda T: launch("hpvg_rowsum_f32", p(T["x"]), p(T["w"]), p(T["out"]), scale, B, C, S)),
                      tag + "rowsum " + wname)
        check("c", r["out"], *V.rowsum64(dz, w, scale), tag + "rowsum " + wname, "rowsum." + wname, key)
        r = all_equal("c", sweep("c", tag + "outer " + wname, {"g": code, "w": w}, {"out": ((B, C, S), f32, None)},
                                 lambda T: launch("hpvg_outer_f32", p(T["g"]), p(T["w"]), p(T["out"]), scale, B, C, S)),
                      tag + "outer " + wname)
        check("c", r["out"], *V.outer64(code, w, scale, S), tag + "outer " + wname, "outer." + wname, key)
    r = all_equal("c", sweep("c", tag + "colsum", {"a": dz, "v": code}, {"out": ((B, S), f32, None)},
                             lambda T: launch("hpvg_colsum_f32", p(T["a"]), p(T["v"]), p(T["out"]), B, C, S)), tag + "colsum")
    check("c", r["out"], *V.colsum64(dz, code), tag + "colsum", "colsum", key)
    r = all_equal("c", sweep("c", tag + "reparam_bern_fwd", {"x": x, "eps": eps}, {"z": ((B, S), f32, None)},
                             lambda T: launch("hpvg_reparam_bern_fwd_f32", p(T["x"]), p(T["eps"]), p(T["z"]), L)), tag + "reparam_bern_fwd")
    check("c", r["z"], *V.reparam_bern_fwd64(x, eps), tag + "reparam_bern", "rbern.fwd", key)
    r = all_equal("c", sweep("c", tag + "reparam_bern_bwd", {"dz": ext, "x": x}, {"dx": ((B, S), f32, None)},
                             lambda T: launch("hpvg_reparam_bern_bwd_f32", p(T["dz"]), p(T["x"]), p(T["dx"]), L)), tag + "reparam_bern_bwd")
    check("c", r["dx"], *V.reparam_bern_bwd64(ext, x), tag + "reparam_bern backward", "rbern.bwd", key)
    r = all_equal("c", sweep("c", tag + "kl_bern_fwd", {"x": x}, {"out": ((1,), f32, None)},
                             lambda T: launch("hpvg_kl_bern_fwd_f32", p(T["x"]), p(T["out"]), *ops._reduce_ws(T["x"].device), L)),
                  tag + "kl_bern_fwd")
    check_scalar("c", r["out"], *V.kl_bern_fwd64(x), tag + "kl_bern", "klbern.fwd", key)
    r = all_equal("c", sweep("c", tag + "kl_bern_bwd", {"gout": gout, "x": x}, {"dx": ((B, S), f32, None)},
                             lambda T: launch("hpvg_kl_bern_bwd_f32", p(T["gout"]), p(T["x"]), p(T["dx"]), L)), tag + "kl_bern_bwd")
    check("c", r["dx"], *V.kl_bern_bwd64(0.83, x), tag + "kl_bern backward", "klbern.bwd", key)


# ================================================================================================ (d) the producer itself
@pytest.mark.parametrize("dims,B", [(3, 1), (3, 2), (2, 1), (2, 2)], ids=["3d-B1", "3d-B2", "2d-B1", "2d-B2"])
def test_critic_step_on_split_batch_output(ops, hplib, lib, dims, B):
    """generated, fake = ops.SplitBatch.apply(x, B) with x of (2B, 3, 3, 5, 7) / (2B, 3, 5, 7): `fake` is a contiguous view off a
    16-byte boundary.  One critic step on it (forward, the gradient penalty with its double backward against a `real`, backward)
    and the same step on fake.clone() - a fresh, aligned allocation - agree bit for bit in the critic outputs, the penalty,
    every parameter gradient of the arena and the gradient SplitBatch.backward returns for x."""
    from hp_vae_gan_amd import optim as hp_optim
    from hp_vae_gan_amd.modules import networks_2d, networks_3d
    sp = (3, 5, 7) if dims == 3 else (5, 7)
    S = E.spatial(sp)
    opt = types.SimpleNamespace(nfc=64, nc_im=3, num_layer=3, ker_size=3, padd_size=1)
    torch.manual_seed(1234 + dims)
    netD = (networks_3d.WDiscriminator3D if dims == 3 else networks_2d.WDiscriminator2D)(opt).to(DEV)
    netD.train()
    arena = hp_optim.ParamArena(netD)
    state = {k: v.clone() for k, v in netD.state_dict().items()}
    g = _gen("critic", dims, B)
    x0 = _randn(g, 2 * B, 3, *sp)
    real = _randn(g, B, 3, *sp)
    alpha = torch.tensor([0.41], device=DEV)

    def step(clone):
        netD.load_state_dict(state)       # the spectral-norm vectors advance with every forward
        ops.weights_changed()
        arena.zero_grad()
        x = OB.embed(x0, 0).requires_grad_(True)
        generated, fake = ops.SplitBatch.apply(x, B)
        assert fake.is_contiguous() and fake.data_ptr() % 16 == (4 * B * 3 * S) % 16 != 0
        assert fake.data_ptr() == x.data_ptr() + 4 * B * 3 * S
        inp = fake.clone() if clone else fake
        assert (inp.data_ptr() % 16 == 0) == clone
        d_real = netD(real)
        d_fake = netD(inp)
        from hp_vae_gan_amd.modules.utils import calc_gradient_penalty
        gp = calc_gradient_penalty(netD, real, inp, 0.1, DEV, alpha=alpha)
        total = ops.MeanScaled.apply(d_real, -1.0) + ops.MeanScaled.apply(d_fake, 1.0) + gp
        total.backward()
        torch.cuda.synchronize()
        _COUNT["d"]["launches"] += 1
        return dict(d_real=d_real.detach(), d_fake=d_fake.detach(), gp=gp.detach(), total=total.detach(), grads=arena.grad.clone(),
                    dx=x.grad.clone(), generated=generated.detach())

    a, b = step(False), step(True)
    for k in a:
        assert torch.isfinite(a[k]).all(), k
        assert torch.equal(a[k], b[k]), "critic step on the offset view vs its aligned clone: %s differs" % k
    _COUNT["d"]["bit"] += 1
    assert float(a["grads"].abs().max()) > 0 and float(a["dx"][B:].abs().max()) > 0
    assert not bool(a["dx"][:B].any())           # nothing flows into `generated`
    ops.weights_changed()


# ================================================================================================ coverage of the module
def _kinds_in_table():
    fwd, wgrad = set(), set()
    for rows in R.KINDS.values():
        for row in rows:
            parts = {q[0]: q[1:] for q in row.split()}
            fwd.update(int(ch) for ch in parts["f"] + parts["d"])
            wgrad.update(int(ch) for ch in parts["w"])
    return fwd, wgrad


def test_coverage_of_the_module(lib):
    """Asserted, not hoped for: the conv launches reached every kernel kind of conv_ref.KINDS; V = 4, 2 and 1 were each chosen
    by the pointer on an S % 4 == 0 shape; both store forms of hpvg_box_copy_f32 ran.  The kinds are host queries, so the first
    half also holds when this test runs alone; the launch records are checked whenever the tests that make them have run."""
    want_f, want_w = _kinds_in_table()
    assert want_f == {0, 1, 2, 3} and want_w == {2, 3, 4}
    static_f, static_w = set(), set()
    for B, (Ci, Co), sp in CONV_CASES:
        T_, H, W, KT = R.kernel_view(sp)
        for mode in FWD_MODES:
            with fwd_mode(lib, mode):
                static_f.update((lib.hpvg_conv_fwd_kernel_kind(B, Ci, Co, T_, H, W, KT), lib.hpvg_conv_fwd_kernel_kind(B, Co, Ci, T_, H, W, KT)))
        for mode in WGRAD_MODES:
            with wgrad_mode(lib, mode):
                static_w.add(lib.hpvg_conv_bwd_weight_kernel_kind(B, Ci, Co, T_, H, W, KT))
    assert static_f >= want_f, "forward / backward-data kinds the cases can reach: %s" % sorted(static_f)
    assert static_w >= want_w, "weight-gradient kinds the cases can reach: %s" % sorted(static_w)
    if _RAN["conv"] == {_conv_id(c) for c in CONV_CASES}:
        assert _FWD_KINDS == static_f and _WGRAD_KINDS == static_w, (sorted(_FWD_KINDS), sorted(_WGRAD_KINDS))
    if _RAN["bn"] == {(tuple(sp), B, g) for sp, B, g in BN_CASES}:
        assert _V_BY_POINTER == {4, 2, 1}, sorted(_V_BY_POINTER)
    if _RAN["box"] == {4, 1, 3}:
        assert _BOX_FORMS == {"16-byte", "element"}, sorted(_BOX_FORMS)
