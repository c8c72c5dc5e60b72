"""The parameter side of a train step - spectral-norm power iteration and backward, the batched weight packs, the gradient clip
and the Adam step - element by element against float64 (tests/param_ref.py): |got - ref| <= tau * A per element,
tau = conv_ref.TAU, A = the error scales derived in param_ref's docstring.

Spectral norm: one SpectralNormWeightBatch.apply over a critic's six layers as sn_weights issues them (param_ref.SN_LAYERS_3D /
_2D, and the same batch with a one-channel last layer), training and eval mode, the backward into fresh tensors and into
the preset .grad slots of a ParamArena with only some layers requiring grad; every stage of the forward is judged against
float64 computed from the kernel's own fp32 output of the stage before.  The single-layer SpectralNormWeight agrees with
the batched launch bit for bit, w_eff included (hpvg_div_scalar_f32 and the in-kernel division are the same correctly rounded
fp32 divide).  Then, through the C ABI, every branch of sn_power_iter_body (float4 with S = 8 ... 1 row slices, the scalar
form by K & 3, by K / 4 > 1024 and by a w or v that is one float into its buffer, Co below S, above 16 and 64, 1024) and of
the backward (the chunk boundaries of SN_CHUNK = 4096, K & 3, Co & 3, each pointer misaligned in turn, a one-chunk layer
beside a 27-chunk layer, accumulate and overwrite mixed), single and batched.
Weight packs: every item of hpvg_conv_pack_weight_batch[_for]_f32 equals the per-layer pack of that weight.
Clip and Adam at n = 1, 1023 and 4096 * 1024 + 3 (the last enters the grid-stride loop of the 4096-block grid), Adam at
t = 1 ... 100000 with the count from the host argument and from device memory, over the real ranges of the video config's
generator arena, and five consecutive FlatAdam steps.

Every launch that takes a workspace runs a second time with every workspace byte set to 0xFF and must reproduce the first
result bit for bit.  The float64 references run through torch's own ops on the GPU."""
import ctypes
import zlib

import pytest
import torch
import torch.nn as nn

import conv_ref as R
import param_ref as P
from launch_common import assert_same, checked, fill_workspaces, print_stats

pytestmark = pytest.mark.gpu

DEV = "cuda"
_STATS = {}
ERR_ARG, ERR_WORKSPACE = -1, -2
BIG = 4096 * 1024 + 3          # elements: past the 4096 blocks x 256 threads x 4 of ew_blocks, so every thread loops


@pytest.fixture(scope="module")
def ops():
    import hp_vae_gan_amd  # noqa: F401
    from hp_vae_gan_amd import ops as _ops
    yield _ops
    print_stats(_STATS, "worst |got - ref| / A per (op, branch) (tau %.0e; '1 rounding': %.3e):" % (P.TAU, P.U1))


@pytest.fixture(scope="module")
def lib(ops):
    from hp_vae_gan_amd import lib as hplib
    assert hplib._CONSTANTS["HPVG_ERR_ARG"] == ERR_ARG and hplib._CONSTANTS["HPVG_ERR_WORKSPACE"] == ERR_WORKSPACE
    return hplib.load()


def _hp():
    from hp_vae_gan_amd import lib as hplib
    return hplib


def _check(got, ref, A, what, quantity, key, tau=P.TAU):
    return checked(_STATS, got, ref, A, what, quantity, key, tau=tau)


def _check_scalar(got, ref, A, what, quantity, key):
    return _check(got.reshape(1), ref.reshape(1), A.reshape(1), what, quantity, key)


def _gen(*key):
    return torch.Generator(device=DEV).manual_seed(zlib.crc32(repr(key).encode()))


def _off(t, k=1):
    """A copy of t that starts k floats into a larger buffer: 4 k bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + k + 3, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0
    view = buf[k:k + t.numel()].view(t.shape)
    view.copy_(t)
    return view


def _ws(ops, nbytes):
    buf = ops.workspace(nbytes, torch.device(DEV, torch.cuda.current_device()))
    return _hp().ptr(buf), buf.numel()


def _arr(ctype, values):
    return (ctype * len(values))(*values)


# ------------------------------------------------------------------------------------------------ spectral norm: drivers
def _sn_data(Co, K, *key):
    g = _gen("sn", Co, K, *key)
    W = torch.randn(Co, K, generator=g, device=DEV) / K ** 0.5
    u = torch.nn.functional.normalize(torch.randn(Co, generator=g, device=DEV), dim=0, eps=1e-12)
    v = torch.nn.functional.normalize(torch.randn(K, generator=g, device=DEV), dim=0, eps=1e-12)
    return W, u, v


def _sn_single(ops, W, u_in, v_in, do_iter, want_uv=True, place_v=None):
    """hpvg_sn_power_iter_f32 -> dict(u, v, sig [2], uv | None); u and v start as copies of u_in / v_in."""
    hp = _hp()
    Co, K = W.shape
    u = u_in.clone()
    v = place_v(v_in) if place_v else v_in.clone()
    sig = torch.full((2,), float("nan"), device=DEV)
    uv = torch.full((Co + K,), float("nan"), device=DEV) if want_uv else None
    hp.call("hpvg_sn_power_iter_f32", hp.ptr(W), hp.ptr(u), hp.ptr(v), hp.ptr(sig[0:1]), hp.ptr(sig[1:2]), hp.ptr(uv), Co, K,
            1 if do_iter else 0, P.SN_EPS, *_ws(ops, 4 * Co), hp.stream())
    torch.cuda.synchronize()
    out = {"u": u, "v": v, "sig": sig}
    if want_uv:
        out["uv"] = uv
    return out


def _sn_batch(ops, items, do_iter):
    """hpvg_sn_power_iter_batch_f32 over items = [(W, u_in, v_in, want_uv)] -> [dict(u, v, sig, uv | None, w_eff)]."""
    hp = _hp()
    n = len(items)
    outs = []
    for W, u_in, v_in, want_uv in items:
        Co, K = W.shape
        o = {"u": u_in.clone(), "v": v_in.clone(), "sig": torch.full((2,), float("nan"), device=DEV),
             "w_eff": torch.full((Co, K), float("nan"), device=DEV)}
        if want_uv:
            o["uv"] = torch.full((Co + K,), float("nan"), device=DEV)
        outs.append(o)
    PA = ctypes.c_void_p * n
    hp.call("hpvg_sn_power_iter_batch_f32", n, PA(*[hp.ptr(it[0]) for it in items]), PA(*[hp.ptr(o["u"]) for o in outs]),
            PA(*[hp.ptr(o["v"]) for o in outs]), PA(*[hp.ptr(o["sig"]) for o in outs]), PA(*[hp.ptr(o.get("uv")) for o in outs]),
            PA(*[hp.ptr(o["w_eff"]) for o in outs]), _arr(ctypes.c_int, [it[0].shape[0] for it in items]),
            _arr(ctypes.c_int, [it[0].shape[1] for it in items]), 1 if do_iter else 0, P.SN_EPS,
            *_ws(ops, 4 * sum(it[0].shape[0] for it in items)), hp.stream())
    torch.cuda.synchronize()
    return outs


def _sn_branch(Co, K, aligned=True):
    """The branch of sn_power_iter_body a launch takes, as the key of the ratio table."""
    K4 = K // 4
    if K % 4 or K4 > 1024 or not aligned:
        return "scalar"
    return "float4 S=%d" % (min(1024 // K4, 8) if K4 <= 512 else 1)


def _check_sn_fwd(tag, key, W, u_in, v_in, o, do_iter):
    """Every stage of one layer's forward against float64 from the stage before's fp32 output (param_ref's docstring)."""
    W2 = W.reshape(W.shape[0], -1)
    Co = W2.shape[0]
    if do_iter:
        _check(o["v"], *P.sn_v64(W2, u_in), tag + "v", "sn.v", key)
        _check(o["u"], *P.sn_u64(W2, o["v"]), tag + "u", "sn.u", key)
    else:
        assert torch.equal(o["u"], u_in) and torch.equal(o["v"], v_in), tag + "u / v changed without an iteration"
    (s, sA), (i, iA) = P.sn_sigma64(W2, o["u"], o["v"])
    _check_scalar(o["sig"][0], s, sA, tag + "sigma", "sn.sigma", key)
    _check_scalar(o["sig"][1], i, iA, tag + "1/sigma", "sn.inv_sigma", key)
    if o.get("uv") is not None:
        assert torch.equal(o["uv"][:Co], o["u"]) and torch.equal(o["uv"][Co:], o["v"]), tag + "the (u, v) copy differs"
    if o.get("w_eff") is not None:
        ref, A = P.sn_weff64(W2, o["sig"][0])
        got = o["w_eff"].reshape(W2.shape)
        _check(got, ref, A, tag + "w_eff", "sn.w_eff", key)
        _check(got, ref, A, tag + "w_eff (one rounding)", "sn.w_eff 1 rounding", key, tau=P.U1)


def _same(a, b, tag):
    for k, v in a.items():
        if isinstance(v, torch.Tensor):
            assert torch.equal(b[k], v), tag + k + " differs"


# ------------------------------------------------------------------------------------------------ spectral norm: real launches
class _Weights(nn.Module):
    def __init__(self, ws):
        super().__init__()
        self.ws = nn.ParameterList([nn.Parameter(w.clone()) for w in ws])


REAL = [("3d", P.SN_LAYERS_3D, 27), ("2d", P.SN_LAYERS_2D, 9), ("3d-tail1", P.SN_TAIL_3D, 27), ("2d-tail1", P.SN_TAIL_2D, 9)]
LIVE = (0, 2, 3, 5)            # the layers that require grad; 1 and 4 are frozen (no (u, v) copy, no backward)


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("name,layers,taps", REAL, ids=[c[0] for c in REAL])
def test_sn_batch_real_launch_against_float64(ops, lib, name, layers, taps, training):
    from hp_vae_gan_amd import optim
    n = len(layers)
    g = _gen("real", name)
    kshape = (3, 3, 3) if taps == 27 else (3, 3)
    ws, us, vs, dws = [], [], [], []
    for Co, K in layers:
        W, u, v = _sn_data(Co, K, name, len(ws))
        ws.append(W.view(Co, K // taps, *kshape))
        us.append(u)
        vs.append(v)
        dws.append(torch.randn(ws[-1].shape, generator=g, device=DEV))
    fresh = [w.clone().requires_grad_(i in LIVE) for i, w in enumerate(ws)]
    mod = _Weights(ws)
    arena = optim.ParamArena(mod)
    params = list(mod.ws)
    for i, p in enumerate(params):
        p.requires_grad_(i in LIVE)
    preset = torch.randn(arena.total, generator=g, device=DEV)

    def interleave(wl, ul, vl):
        return [t for trio in zip(wl, ul, vl) for t in trio]

    def launch():
        out = {}
        u1, v1 = [u.clone() for u in us], [v.clone() for v in vs]
        outs = ops.SpectralNormWeightBatch.apply(training, P.SN_EPS, *interleave(fresh, u1, v1))
        saved = outs[LIVE[0]].grad_fn.saved_tensors
        out["sig"] = saved[0].clone()
        uvs = saved[1 + n:1 + 2 * n]
        grads = torch.autograd.grad([outs[i] for i in LIVE], [fresh[i] for i in LIVE], [dws[i] for i in LIVE])
        for j, i in enumerate(LIVE):
            out["dw%d" % i] = grads[j]
        for i in range(n):
            out["w%d" % i], out["u%d" % i], out["v%d" % i] = outs[i].detach(), u1[i], v1[i]
            assert (uvs[i] is not None) == (i in LIVE)
            if uvs[i] is not None:
                out["uv%d" % i] = uvs[i].clone()
        # the same launch on the arena's parameters, its backward straight into the preset .grad slots
        arena.grad.copy_(preset)
        u2, v2 = [u.clone() for u in us], [v.clone() for v in vs]
        outs2 = ops.SpectralNormWeightBatch.apply(training, P.SN_EPS, *interleave(params, u2, v2))
        torch.autograd.backward([outs2[i] for i in LIVE], [dws[i] for i in LIVE])
        for i, p in enumerate(params):
            o, cnt = arena.range[id(p)]
            assert p.grad.data_ptr() == arena.grad.data_ptr() + 4 * o, "autograd replaced the .grad slot of layer %d" % i
            assert torch.equal(outs2[i], outs[i]) and torch.equal(u2[i], u1[i]) and torch.equal(v2[i], v1[i])
        out["slots"] = arena.grad.clone()
        torch.cuda.synchronize()
        return out

    o = launch()
    mode = "train" if training else "eval"
    for i, (Co, K) in enumerate(layers):
        tag = "%s %s layer %d (%d, %d): " % (name, mode, i, Co, K)
        key = _sn_branch(Co, K)
        lo = {"u": o["u%d" % i], "v": o["v%d" % i], "sig": o["sig"][i], "uv": o.get("uv%d" % i), "w_eff": o["w%d" % i]}
        _check_sn_fwd(tag, key, ws[i], us[i], vs[i], lo, training)
        off, cnt = arena.range[id(params[i])]
        slot, pre = o["slots"][off:off + cnt].view(ws[i].shape), preset[off:off + cnt].view(ws[i].shape)
        if i in LIVE:
            bkey = "batch " + _bwd_branch(Co, K, batched=True)
            ref, A = P.sn_bwd64(dws[i], ws[i], lo["sig"][0], lo["u"], lo["v"])
            _check(o["dw%d" % i], ref, A, tag + "dW_orig", "sn.bwd", bkey)
            ref, A = P.sn_bwd64(dws[i], ws[i], lo["sig"][0], lo["u"], lo["v"], preset=pre)
            _check(slot, ref, A, tag + "dW_orig into the preset slot", "sn.bwd.slot", bkey)
        else:
            assert torch.equal(slot, pre), tag + "the .grad slot of a frozen layer changed"
        # the single-layer form: bit for bit
        w1 = ws[i].clone().requires_grad_(True)
        u1, v1 = us[i].clone(), vs[i].clone()
        we = ops.SpectralNormWeight.apply(w1, u1, v1, training, P.SN_EPS)
        _, uv1, sig1 = we.grad_fn.saved_tensors
        assert torch.equal(we, lo["w_eff"]), tag + "w_eff of the single-layer form differs from the batched launch"
        assert torch.equal(u1, lo["u"]) and torch.equal(v1, lo["v"]) and torch.equal(sig1, lo["sig"]), tag + "single vs batched"
        if lo["uv"] is not None:
            assert torch.equal(uv1, lo["uv"])
        (dw1,) = torch.autograd.grad(we, [w1], dws[i])
        ref, A = P.sn_bwd64(dws[i], ws[i], sig1[0], u1, v1)
        _check(dw1, ref, A, tag + "dW_orig, single-layer form", "sn.bwd", "single " + _bwd_branch(Co, K, batched=False, uv_co=Co))
    pad = torch.ones(arena.total, dtype=torch.bool, device=DEV)
    for p in params:
        off, cnt = arena.range[id(p)]
        pad[off:off + cnt] = False
    assert torch.equal(o["slots"][pad], preset[pad]), "the arena's padding changed"
    fill_workspaces(ops)
    assert_same(o, launch(), "%s %s: " % (name, mode))


# ------------------------------------------------------------------------------------------------ spectral norm: branch edges
KS = (4, 512, 516, 2048, 2052, 4096, 4100, 81, 2106)
COS = (1, 3, 16, 17, 78, 1024)
EDGES = sorted({(Co, K) for K in KS for Co in (3, 17)} | {(Co, K) for Co in COS for K in (516, 81)}
               | {(78, 2106), (1024, 2052), (1024, 4100), (1, 4), (1, 1728)})


@pytest.mark.parametrize("Co,K", EDGES, ids=["%dx%d-%s" % (c, k, _sn_branch(c, k).replace(" ", "")) for c, k in EDGES])
def test_sn_forward_branch_edges(ops, lib, Co, K):
    """Single and batched (n = 1) launch of one layer, with and without the iteration, with and without the (u, v) copy."""
    W, u_in, v_in = _sn_data(Co, K, "edge")
    key = _sn_branch(Co, K)
    tag = "(%d, %d) %s: " % (Co, K, key)

    def launch():
        out = {}
        for do_iter in (1, 0):
            s = _sn_single(ops, W, u_in, v_in, do_iter, want_uv=bool(do_iter))
            (b,) = _sn_batch(ops, [(W, u_in, v_in, not do_iter)], do_iter)
            for k, v in s.items():
                out["single%d.%s" % (do_iter, k)] = v
            for k, v in b.items():
                out["batch%d.%s" % (do_iter, k)] = v
        return out

    o = launch()
    for do_iter in (1, 0):
        s = {k.split(".")[1]: v for k, v in o.items() if k.startswith("single%d." % do_iter)}
        b = {k.split(".")[1]: v for k, v in o.items() if k.startswith("batch%d." % do_iter)}
        _check_sn_fwd(tag + ("" if do_iter else "no iteration, "), key, W, u_in, v_in, s, do_iter)
        _check_sn_fwd(tag + "batched, " + ("" if do_iter else "no iteration, "), key, W, u_in, v_in, b, do_iter)
        for k in ("u", "v", "sig"):
            assert torch.equal(s[k], b[k]), tag + "%s differs between the single and the batched launch" % k
    fill_workspaces(ops)
    assert_same(o, launch(), tag)


MISALIGNED = [(3, 512), (17, 2048), (16, 4096), (78, 516), (1, 1728)]


@pytest.mark.parametrize("which", ["w", "v"])
@pytest.mark.parametrize("Co,K", MISALIGNED, ids=["%dx%d" % c for c in MISALIGNED])
def test_sn_forward_misaligned_takes_the_scalar_form(ops, lib, Co, K, which):
    """The same data with w, then v, one float into a larger buffer: a float4 shape on the scalar form.  v is judged
    against the aligned run's reference (the same float64 of (W, u_in)); the later stages against float64 from this
    run's own fp32 v and u, as everywhere (the aligned run's v differs from this one's by a rounding, which a reference
    built on it would carry into u and sigma)."""
    W, u_in, v_in = _sn_data(Co, K, "edge")
    assert _sn_branch(Co, K).startswith("float4")
    tag = "(%d, %d) %s one float off: " % (Co, K, which)
    Wm = _off(W) if which == "w" else W
    assert (Wm.data_ptr() % 16 != 0) == (which == "w")
    place = _off if which == "v" else None

    def launch():
        return {"%d.%s" % (do_iter, k): t for do_iter in (1, 0)
                for k, t in _sn_single(ops, Wm, u_in, v_in, do_iter, place_v=place).items()}

    o = launch()
    for do_iter in (1, 0):
        s = {k[2:]: t for k, t in o.items() if k.startswith("%d." % do_iter)}
        assert (s["v"].data_ptr() % 16 != 0) == (which == "v")
        _check_sn_fwd(tag, "scalar (misaligned)", W, u_in, v_in, s, do_iter)
    fill_workspaces(ops)
    assert_same(o, launch(), tag)
    a = _sn_single(ops, W, u_in, v_in, 1)
    vr, vA = P.sn_v64(W, u_in)
    _check(a["v"], vr, vA, tag + "aligned v", "sn.v", _sn_branch(Co, K))
    # batched: the same misaligned layer beside an aligned one
    hp = _hp()
    W2, u2, v2 = _sn_data(16, 512, "edge")
    outs = []
    for Wx, ux, vx in ((Wm, u_in, v_in), (W2, u2, v2)):
        Cx, Kx = Wx.shape
        outs.append({"u": ux.clone(), "v": (place(vx) if place and Wx is Wm else vx.clone()),
                     "sig": torch.empty(2, device=DEV), "uv": torch.empty(Cx + Kx, device=DEV),
                     "w_eff": torch.empty(Cx, Kx, device=DEV)})
    PA = ctypes.c_void_p * 2
    hp.call("hpvg_sn_power_iter_batch_f32", 2, PA(hp.ptr(Wm), hp.ptr(W2)), PA(*[hp.ptr(x["u"]) for x in outs]),
            PA(*[hp.ptr(x["v"]) for x in outs]), PA(*[hp.ptr(x["sig"]) for x in outs]), PA(*[hp.ptr(x["uv"]) for x in outs]),
            PA(*[hp.ptr(x["w_eff"]) for x in outs]), _arr(ctypes.c_int, [Co, 16]), _arr(ctypes.c_int, [K, 512]), 1, P.SN_EPS,
            *_ws(ops, 4 * (Co + 16)), hp.stream())
    torch.cuda.synchronize()
    _check_sn_fwd(tag + "batched, ", "scalar (misaligned)", W, u_in, v_in, outs[0], 1)
    _check_sn_fwd(tag + "batched, aligned neighbour ", _sn_branch(16, 512), W2, u2, v2, outs[1], 1)


def test_sn_forward_batch_of_eight_and_refusals(ops, lib):
    """n = 8 layers mixing float4 and scalar shapes, some without a (u, v) copy; n = 9 and Co = 1025 are refused."""
    hp = _hp()
    assert hp.SN_BATCH_MAX == 8
    shapes = [(64, 81), (64, 1728), (3, 512), (17, 2052), (1, 1728), (16, 4100), (78, 2106), (5, 4)]
    data = [_sn_data(Co, K, "eight", i) for i, (Co, K) in enumerate(shapes)]
    items = [(W, u, v, i % 3 != 1) for i, (W, u, v) in enumerate(data)]

    def launch():
        out = {}
        for do_iter in (1, 0):
            for i, b in enumerate(_sn_batch(ops, items, do_iter)):
                for k, v in b.items():
                    out["%d.%d.%s" % (do_iter, i, k)] = v
        return out

    o = launch()
    for do_iter in (1, 0):
        for i, (Co, K) in enumerate(shapes):
            b = {k.split(".")[2]: v for k, v in o.items() if k.startswith("%d.%d." % (do_iter, i))}
            assert ("uv" in b) == (i % 3 != 1)
            _check_sn_fwd("batch of 8, layer %d (%d, %d): " % (i, Co, K), _sn_branch(Co, K), *data[i], b, do_iter)
            s = _sn_single(ops, *data[i], do_iter)
            for k in ("u", "v", "sig"):
                assert torch.equal(s[k], b[k]), "layer %d: %s differs between the single and the batched launch" % (i, k)
    fill_workspaces(ops)
    assert_same(o, launch(), "batch of 8: ")

    W, u, v = data[2]
    nine = [(W, u.clone(), v.clone(), torch.empty(2, device=DEV), torch.empty_like(W)) for _ in range(9)]
    PA = ctypes.c_void_p * 9
    wsp = _ws(ops, 4 * 9 * 3)
    rc = lib.hpvg_sn_power_iter_batch_f32(9, PA(*[hp.ptr(t[0]) for t in nine]), PA(*[hp.ptr(t[1]) for t in nine]),
                                          PA(*[hp.ptr(t[2]) for t in nine]), PA(*[hp.ptr(t[3]) for t in nine]), None,
                                          PA(*[hp.ptr(t[4]) for t in nine]), _arr(ctypes.c_int, [3] * 9),
                                          _arr(ctypes.c_int, [512] * 9), 1, P.SN_EPS, *wsp, hp.stream())
    assert rc == ERR_ARG
    Wb, ub, vb = _sn_data(1025, 4, "refused")
    sig = torch.empty(2, device=DEV)
    rc = lib.hpvg_sn_power_iter_f32(hp.ptr(Wb), hp.ptr(ub), hp.ptr(vb), hp.ptr(sig[0:1]), hp.ptr(sig[1:2]), None, 1025, 4, 1,
                                    P.SN_EPS, *_ws(ops, 4 * 1025), hp.stream())
    assert rc == ERR_ARG
    PA1 = ctypes.c_void_p * 1
    weff = torch.empty_like(Wb)
    rc = lib.hpvg_sn_power_iter_batch_f32(1, PA1(hp.ptr(Wb)), PA1(hp.ptr(ub)), PA1(hp.ptr(vb)), PA1(hp.ptr(sig)), None,
                                          PA1(hp.ptr(weff)), _arr(ctypes.c_int, [1025]), _arr(ctypes.c_int, [4]), 1, P.SN_EPS,
                                          *_ws(ops, 4 * 1025), hp.stream())
    assert rc == ERR_ARG
    # a short workspace
    W, u, v = data[0]
    rc = lib.hpvg_sn_power_iter_f32(hp.ptr(W), hp.ptr(u.clone()), hp.ptr(v.clone()), hp.ptr(sig[0:1]), hp.ptr(sig[1:2]), None,
                                    64, 81, 1, P.SN_EPS, _ws(ops, 256)[0], 4 * 64 - 1, hp.stream())
    assert rc == ERR_WORKSPACE
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ spectral norm backward
def _bwd_branch(Co, K, batched, uv_co=None, aligned=True):
    """float4 or scalar: the batched form needs K & 3 == 0, Co & 3 == 0 (its v is uv + Co) and four aligned pointers; the
    single form K & 3 == 0 and an aligned v (uv_co: v is the tail of a (u, v) copy with that many u entries)."""
    if K % 4 or not aligned:
        return "scalar"
    if batched:
        return "float4" if Co % 4 == 0 else "scalar"
    return "float4" if (uv_co is None or uv_co % 4 == 0) else "scalar"


def _bwd_data(Co, K, *key):
    g = _gen("bwd", Co, K, *key)
    W = torch.randn(Co, K, generator=g, device=DEV) / K ** 0.5
    dW = torch.randn(Co, K, generator=g, device=DEV)
    uv = torch.cat([torch.nn.functional.normalize(torch.randn(Co, generator=g, device=DEV), dim=0),
                    torch.nn.functional.normalize(torch.randn(K, generator=g, device=DEV), dim=0)])
    sigma = 0.5 + torch.rand(1, generator=g, device=DEV)
    preset = torch.randn(Co, K, generator=g, device=DEV)
    return {"W": W, "dW": dW, "uv": uv, "sigma": sigma, "preset": preset, "Co": Co, "K": K}


def _bwd_single(ops, d, accumulate, split_uv=False):
    """hpvg_sn_bwd_f32; u and v are the head and tail of the (u, v) copy, or (split_uv) buffers of their own."""
    hp = _hp()
    Co, K = d["Co"], d["K"]
    u, v = d["uv"][:Co], d["uv"][Co:]
    if split_uv:
        u, v = u.clone(), v.clone()
    out = d["preset"].clone() if accumulate else torch.full((Co, K), float("nan"), device=DEV)
    hp.call("hpvg_sn_bwd_f32", hp.ptr(d["dW"]), hp.ptr(d["W"]), hp.ptr(u), hp.ptr(v), hp.ptr(d["sigma"]), hp.ptr(out),
            1 if accumulate else 0, *_ws(ops, hp.call("hpvg_sn_bwd_ws_bytes", Co, K)), Co, K, hp.stream())
    torch.cuda.synchronize()
    return out


def _bwd_batch(ops, ds, accumulate, outs=None):
    hp = _hp()
    n = len(ds)
    if outs is None:
        outs = [d["preset"].clone() if a else torch.full((d["Co"], d["K"]), float("nan"), device=DEV) for d, a in zip(ds, accumulate)]
    PA = ctypes.c_void_p * n
    need = sum(hp.call("hpvg_sn_bwd_ws_bytes", d["Co"], d["K"]) for d in ds)
    hp.call("hpvg_sn_bwd_batch_f32", n, PA(*[hp.ptr(d["dW"]) for d in ds]), PA(*[hp.ptr(d["W"]) for d in ds]),
            PA(*[hp.ptr(d["uv"]) for d in ds]), PA(*[hp.ptr(d["sigma"]) for d in ds]), PA(*[hp.ptr(o) for o in outs]),
            _arr(ctypes.c_int, [1 if a else 0 for a in accumulate]), _arr(ctypes.c_int, [d["Co"] for d in ds]),
            _arr(ctypes.c_int, [d["K"] for d in ds]), *_ws(ops, need), hp.stream())
    torch.cuda.synchronize()
    return outs


def _check_bwd(tag, key, d, got, accumulate, quantity="sn.bwd"):
    Co = d["Co"]
    ref, A = P.sn_bwd64(d["dW"], d["W"], d["sigma"], d["uv"][:Co], d["uv"][Co:], preset=d["preset"] if accumulate else None)
    _check(got, ref, A, tag + ("accumulate" if accumulate else "overwrite"), quantity + (".slot" if accumulate else ""), key)


# Co * K = 4095, 4096, 4097, 4100, 8192 around SN_CHUNK = 4096; K & 3 != 0; Co & 3 != 0 with K & 3 == 0 (a uv with Co = 1,
# 2, 5, 25: the batched form goes scalar, the single form only when v = uv + Co is misaligned); the wide configs' (78, 2106)
BWD_EDGES = [(1, 4095), (3, 1365), (4, 1024), (1, 4096), (1, 4097), (1, 4100), (25, 164), (8, 1024), (2, 4096), (5, 1640),
             (64, 81), (78, 2106), (4, 4), (1, 1728)]


@pytest.mark.parametrize("Co,K", BWD_EDGES, ids=["%dx%d" % c for c in BWD_EDGES])
def test_sn_backward_branch_edges(ops, lib, Co, K):
    d = _bwd_data(Co, K)
    tag = "(%d, %d) backward, " % (Co, K)

    def launch():
        out = {}
        for acc in (0, 1):
            out["single%d" % acc] = _bwd_single(ops, d, acc)
            out["split%d" % acc] = _bwd_single(ops, d, acc, split_uv=True)
            (out["batch%d" % acc],) = _bwd_batch(ops, [d], [acc])
        return out

    o = launch()
    for acc in (0, 1):
        _check_bwd(tag + "single, ", "single " + _bwd_branch(Co, K, False, uv_co=Co), d, o["single%d" % acc], acc)
        _check_bwd(tag + "single, v in its own buffer, ", "single " + _bwd_branch(Co, K, False), d, o["split%d" % acc], acc)
        _check_bwd(tag + "batched, ", "batch " + _bwd_branch(Co, K, True), d, o["batch%d" % acc], acc)
    fill_workspaces(ops)
    assert_same(o, launch(), tag)


@pytest.mark.parametrize("which", ["dW", "W", "uv", "out"])
def test_sn_backward_misaligned_pointers(ops, lib, which):
    """Each of dweff, worig, uv and dworig one float into a larger buffer in turn, on a two-chunk float4 shape."""
    hp = _hp()
    Co, K = 8, 1024
    d = _bwd_data(Co, K, "mis")
    m = dict(d)
    if which != "out":
        m[which] = _off(d[which])
        assert m[which].data_ptr() % 16 == 4
    tag = "(8, 1024) backward, %s one float off, " % which

    def fresh_out(acc):
        t = d["preset"].clone() if acc else torch.full((Co, K), float("nan"), device=DEV)
        return _off(t) if which == "out" else t

    def launch():
        res = {}
        for acc in (0, 1):
            (res["batch%d" % acc],) = _bwd_batch(ops, [m], [acc], outs=[fresh_out(acc)])
            # single form: u and v are the head and tail of uv (Co = 8: v is as aligned as uv)
            out = fresh_out(acc)
            hp.call("hpvg_sn_bwd_f32", hp.ptr(m["dW"]), hp.ptr(m["W"]), hp.ptr(m["uv"][:Co]), hp.ptr(m["uv"][Co:]),
                    hp.ptr(m["sigma"]), hp.ptr(out), acc, *_ws(ops, hp.call("hpvg_sn_bwd_ws_bytes", Co, K)), Co, K, hp.stream())
            torch.cuda.synchronize()
            res["single%d" % acc] = out
        return res

    o = launch()
    for acc in (0, 1):
        assert (o["batch%d" % acc].data_ptr() % 16 != 0) == (which == "out")
        _check_bwd(tag + "batched, ", "batch scalar (misaligned)", d, o["batch%d" % acc], acc)
        _check_bwd(tag + "single, ", "single scalar (misaligned)", d, o["single%d" % acc], acc)
    fill_workspaces(ops)
    assert_same(o, launch(), tag)


def test_sn_backward_mixed_batch_and_short_workspace(ops, lib):
    """(1, 1728) beside (64, 1728): 26 of the short layer's 27 workgroups return early; accumulate and overwrite mixed, a
    float4 and a scalar layer mixed; a workspace one byte short is refused by both forms."""
    hp = _hp()
    shapes = [(1, 1728), (64, 1728), (64, 81), (4, 1024), (64, 1728), (25, 164)]
    ds = [_bwd_data(Co, K, "mixed", i) for i, (Co, K) in enumerate(shapes)]
    acc = [1, 0, 1, 0, 1, 0]

    def launch():
        return {"o%d" % i: t for i, t in enumerate(_bwd_batch(ops, ds, acc))}

    o = launch()
    for i, (Co, K) in enumerate(shapes):
        _check_bwd("mixed batch, layer %d (%d, %d), " % (i, Co, K), "batch " + _bwd_branch(Co, K, True), ds[i], o["o%d" % i], acc[i])
    fill_workspaces(ops)
    assert_same(o, launch(), "mixed batch: ")
    for flip in ([0, 1], [1, 0]):
        pair = _bwd_batch(ops, ds[:2], flip)
        for i in (0, 1):
            _check_bwd("pair %s, layer %d, " % (flip, i), "batch " + _bwd_branch(*shapes[i], True), ds[i], pair[i], flip[i])

    d = ds[1]
    need = hp.call("hpvg_sn_bwd_ws_bytes", 64, 1728)
    assert need == 27 * 8
    out = torch.zeros(64, 1728, device=DEV)
    wsp = _ws(ops, need)[0]
    rc = lib.hpvg_sn_bwd_f32(hp.ptr(d["dW"]), hp.ptr(d["W"]), hp.ptr(d["uv"][:64]), hp.ptr(d["uv"][64:]), hp.ptr(d["sigma"]),
                             hp.ptr(out), 0, wsp, need - 1, 64, 1728, hp.stream())
    assert rc == ERR_WORKSPACE
    PA = ctypes.c_void_p * 2
    outs = [torch.zeros(1, 1728, device=DEV), out]
    rc = lib.hpvg_sn_bwd_batch_f32(2, PA(*[hp.ptr(x["dW"]) for x in ds[:2]]), PA(*[hp.ptr(x["W"]) for x in ds[:2]]),
                                   PA(*[hp.ptr(x["uv"]) for x in ds[:2]]), PA(*[hp.ptr(x["sigma"]) for x in ds[:2]]),
                                   PA(*[hp.ptr(x) for x in outs]), _arr(ctypes.c_int, [0, 0]), _arr(ctypes.c_int, [1, 64]),
                                   _arr(ctypes.c_int, [1728, 1728]), wsp, need + 8 - 1, hp.stream())
    assert rc == ERR_WORKSPACE
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ weight packs
WINO2D_GEOM = (1, 3, 96, 128)      # hpvg_conv_wants_wino2d(C = 64, KT = 3) = 1: the _for pack carries the two-axis section
PLAIN_GEOM = (1, 4, 18, 33)        # = 0: it leaves the section out


@pytest.mark.parametrize("n", [1, 2, 16])
@pytest.mark.parametrize("KT", [1, 3])
@pytest.mark.parametrize("C", [8, 64])
def test_batched_weight_packs_equal_the_per_layer_packs(ops, lib, C, KT, n):
    hp = _hp()
    assert hp.PACK_BATCH_MAX == 16
    g = _gen("pack", C, KT, n)
    kshape = (3, 3, 3) if KT == 3 else (3, 3)
    ws = [torch.randn(C, C, *kshape, generator=g, device=DEV) for _ in range(n)]
    flips = [(i * 7 // 3) % 2 for i in range(n)] if n > 1 else [1]
    PA = ctypes.c_void_p * n
    st = hp.stream()
    geoms = [None] + ([WINO2D_GEOM, PLAIN_GEOM] if (C, KT) == (64, 3) else [PLAIN_GEOM])
    for geom in geoms:
        if geom is None:
            nfl = hp.call("hpvg_conv_wpack_floats", C, C, KT)
        else:
            nfl = hp.call("hpvg_conv_wpack_floats_for", C, C, KT, *geom)
            want = lib.hpvg_conv_wants_wino2d(geom[0], C, C, geom[1], geom[2], geom[3], KT)
            assert want == (1 if (C, KT, geom) == (64, 3, WINO2D_GEOM) else 0)
            assert (nfl == hp.call("hpvg_conv_wpack_floats", C, C, KT)) == (want == 1 or (C, KT) != (64, 3))
        batch = [torch.full((nfl + 64,), float("nan"), device=DEV) for _ in range(n)]
        one = [torch.full((nfl + 64,), float("nan"), device=DEV) for _ in range(n)]
        if geom is None:
            hp.call("hpvg_conv_pack_weight_batch_f32", n, PA(*[hp.ptr(w) for w in ws]), PA(*[hp.ptr(t) for t in batch]),
                    _arr(ctypes.c_int, flips), C, KT, st)
            for w, f, t in zip(ws, flips, one):
                hp.call("hpvg_conv_pack_weight_f32", hp.ptr(w), None, hp.ptr(t), C, C, KT, f, st)
        else:
            hp.call("hpvg_conv_pack_weight_batch_for_f32", n, PA(*[hp.ptr(w) for w in ws]), PA(*[hp.ptr(t) for t in batch]),
                    _arr(ctypes.c_int, flips), C, KT, *geom, st)
            for w, f, t in zip(ws, flips, one):
                hp.call("hpvg_conv_pack_weight_for_f32", hp.ptr(w), None, hp.ptr(t), C, C, KT, f, *geom, st)
        torch.cuda.synchronize()
        for i in range(n):
            tag = "C=%d KT=%d n=%d geometry %s item %d (flip %d): " % (C, KT, n, geom, i, flips[i])
            assert not bool(torch.isnan(one[i][:nfl]).any()), tag + "the per-layer pack left a NaN inside the pack"
            assert not bool(torch.isnan(batch[i][:nfl]).any()), tag + "the batched pack left a NaN inside the pack"
            assert torch.equal(batch[i][:nfl], one[i][:nfl]), tag + "the batched pack differs from the per-layer pack"
            assert bool(torch.isnan(batch[i][nfl:]).all()) and bool(torch.isnan(one[i][nfl:]).all()), tag + "wrote past the pack"
    if n == 2:
        t17 = [torch.empty(nfl, device=DEV) for _ in range(17)]
        PA17 = ctypes.c_void_p * 17
        args = (17, PA17(*[hp.ptr(ws[0])] * 17), PA17(*[hp.ptr(t) for t in t17]), _arr(ctypes.c_int, [0] * 17), C, KT)
        assert lib.hpvg_conv_pack_weight_batch_f32(*args, st) == ERR_ARG
        assert lib.hpvg_conv_pack_weight_batch_for_f32(*args, *PLAIN_GEOM, st) == ERR_ARG


@pytest.mark.parametrize("geom", [WINO2D_GEOM, PLAIN_GEOM], ids=["wino2d", "plain"])
def test_conv_from_the_geometry_pack_equals_conv_from_the_full_pack(ops, lib, geom):
    hp = _hp()
    C, KT = 64, 3
    B, T, H, W = geom
    g = _gen("packconv", geom)
    w = torch.randn(C, C, 3, 3, 3, generator=g, device=DEV) / (27 * C) ** 0.5
    x = torch.randn(B, C, T, H, W, generator=g, device=DEV)
    full = torch.empty(hp.call("hpvg_conv_wpack_floats", C, C, KT), device=DEV)
    part = torch.empty(hp.call("hpvg_conv_wpack_floats_for", C, C, KT, *geom), device=DEV)
    PA = ctypes.c_void_p * 1
    hp.call("hpvg_conv_pack_weight_f32", hp.ptr(w), None, hp.ptr(full), C, C, KT, 0, hp.stream())
    hp.call("hpvg_conv_pack_weight_batch_for_f32", 1, PA(hp.ptr(w)), PA(hp.ptr(part)), _arr(ctypes.c_int, [0]), C, KT, *geom,
            hp.stream())
    ys = []
    for k, wp in enumerate((full, part, full, part)):
        if k == 2:
            fill_workspaces(ops)
        y = torch.full((B, C, T, H, W), float("nan"), device=DEV)
        nws = hp.call("hpvg_conv_fwd_ws_bytes", B, C, C, T, H, W, KT)
        wsp = _ws(ops, nws) if nws else (None, 0)
        hp.call("hpvg_conv_fwd_f32", hp.ptr(x), hp.ptr(wp), None, None, None, 0, hp.ptr(y), 0, None, *wsp, B, C, C, T, H, W, KT,
                hp.stream())
        torch.cuda.synchronize()
        ys.append(y)
    assert not bool(torch.isnan(ys[0]).any())
    assert torch.equal(ys[0], ys[1]), "the conv from the geometry-aware pack differs from the conv from the full pack"
    assert torch.equal(ys[2], ys[0]) and torch.equal(ys[3], ys[0]), "differs after the workspace was filled with 0xFF"
    ref, A = R.conv_fwd64_taps(x[:, :, :, :8, :16].contiguous(), w)    # a corner of it against float64: the pack is the layer's
    _check(ys[0][:, :, :, :6, :14], ref[:, :, :, :6, :14], A[:, :, :, :6, :14], "conv from the pack", "pack.conv",
           "wino2d" if geom == WINO2D_GEOM else "plain")


# ------------------------------------------------------------------------------------------------ clip
@pytest.mark.parametrize("with_info", [True, False], ids=["info", "noinfo"])
@pytest.mark.parametrize("case", ["above", "below", "zero"])
@pytest.mark.parametrize("n", [1, 1023, BIG], ids=["n1", "n1023", "gridstride"])
def test_clip_against_float64(ops, lib, n, case, with_info):
    g0 = _gen("clip", n, case)
    max_norm = 5.0
    grad = torch.randn(n, generator=g0, device=DEV)
    if case == "zero":
        grad.zero_()
    else:
        want = 20.0 if case == "above" else 1.5
        grad = grad * (want / float(grad.double().norm())) if n > 1 else torch.full((1,), want, device=DEV)

    def launch():
        g = grad.clone()
        sq = ops.sqsum(g)
        info = torch.full((2,), float("nan"), device=DEV) if with_info else None
        ops.clip_scale_(g, sq, max_norm, info)
        torch.cuda.synchronize()
        return {"g": g, "sq": sq.clone(), "info": info}

    o = launch()
    g, sq, info = o["g"], o["sq"], o["info"]
    fill_workspaces(ops)
    assert_same(o, launch(), "clip %s n=%d: " % (case, n))
    key = "n=%d" % n
    _check(sq, *[t.reshape(1) for t in _sq64(grad)], "sqsum", "clip.sqsum", key)
    (total, tA), (coef, cA) = P.clip64(sq, max_norm)
    assert (float(coef) < 1) == (case == "above")
    assert not bool(torch.isnan(g).any())
    if with_info:
        _check_scalar(info[1], total, tA, "clip %s n=%d: total" % (case, n), "clip.total", key)
        _check_scalar(info[0], coef, cA, "clip %s n=%d: coef" % (case, n), "clip.coef", key)
        if case != "above":
            assert float(info[0]) == 1.0
    if case == "above":
        _check(g, *P.clip_apply64(grad, coef), "clip above n=%d: g" % n, "clip.g", key)
    else:
        assert torch.equal(g, grad), "clip %s n=%d: coef = 1 must return g bit for bit" % (case, n)


def _sq64(x):
    v = x.double().pow(2).sum()
    return v, v.clone()


# ------------------------------------------------------------------------------------------------ Adam
HP = dict(lr=5e-4, beta2=0.999, eps=1e-8)
TS = (1, 2, 3, 10, 1000, 100000)


def _adam_state(n, *key):
    """p (a quarter exactly 0: the update judged alone), g over five decades, m, v >= 0; one block with g = m = v = 0."""
    g0 = _gen("adam", n, *key)
    p = torch.randn(n, generator=g0, device=DEV)
    p[: max(1, n // 4)] = 0        # (n = 1: p = 0, or conv_ref.check's global-maximum measure would judge u |p| by |upd|)
    g = torch.randn(n, generator=g0, device=DEV) * 10.0 ** torch.randint(-4, 1, (n,), generator=g0, device=DEV).float()
    m = 0.1 * torch.randn(n, generator=g0, device=DEV)
    v = (0.1 * torch.randn(n, generator=g0, device=DEV)) ** 2
    z = slice(n // 2, n // 2 + max(1, n // 8)) if n > 1 else slice(0, 0)
    g[z], m[z], v[z] = 0, 0, 0
    return p, g, m, v, z


def _check_adam(tag, key, before, after, t, lr, beta1):
    """One step: m', v' and the update p - p' (param_ref's docstring); the update also on the p = 0 elements alone."""
    p, g, m, v = before
    p1, m1, v1 = after
    (mr, mA), (vr, vA) = P.adam_moments64(g, m, v, beta1, HP["beta2"])
    _check(m1, mr, mA, tag + "m", "adam.m", key)
    _check(v1, vr, vA, tag + "v", "adam.v", key)
    ur, uA = P.adam_update64(p, m1, v1, t, lr, beta1, HP["beta2"], HP["eps"])
    upd = p.double() - p1.double()
    _check(upd, ur, uA, tag + "update p - p'", "adam.update", key)
    zero = p == 0
    if bool(zero.any()):
        _check(upd[zero], ur[zero], uA[zero], tag + "update where p = 0", "adam.update p=0", key)


@pytest.mark.parametrize("beta1", [0.5, 0.9])
@pytest.mark.parametrize("t", TS)
@pytest.mark.parametrize("n", [1, 1023, BIG], ids=["n1", "n1023", "gridstride"])
def test_adam_single_step_against_float64(ops, lib, n, t, beta1):
    """One step from random moments with the count from the host argument (step_dev NULL) and from device memory (the host
    argument then holds another count: a kernel reading the wrong source fails); both must agree bit for bit."""
    p, g, m, v, z = _adam_state(n, t, beta1)
    tag = "Adam n=%d t=%d beta1=%.1f: " % (n, t, beta1)
    key = "t=%d b1=%.1f" % (t, beta1)
    runs = []
    for source in ("host", "device"):
        p1, m1, v1 = p.clone(), m.clone(), v.clone()
        if source == "host":
            ops.adam_step_(p1, g, m1, v1, HP["lr"], beta1, HP["beta2"], HP["eps"], t, None)
        else:
            t_dev = torch.tensor([t], dtype=torch.int32, device=DEV)
            ops.adam_step_(p1, g, m1, v1, HP["lr"], beta1, HP["beta2"], HP["eps"], t + 7 if t != 3 else 1, t_dev)
            assert int(t_dev.item()) == t
        torch.cuda.synchronize()
        runs.append((p1, m1, v1))
    for a, b in zip(*runs):
        assert torch.equal(a, b), tag + "the step counted on the host differs from the step counted on the device"
    _check_adam(tag, key, (p, g, m, v), runs[0], t, HP["lr"], beta1)
    p1, m1, v1 = runs[0]
    assert torch.equal(p1[z], p[z]) and float(m1[z].abs().sum()) == 0.0 and float(v1[z].abs().sum()) == 0.0, \
        tag + "g = m = v = 0 must leave p as it is"


def test_adam_over_the_generator_arena(ops, lib):
    """FlatAdam.step() over the video config's stage-1 generator arena: three ranges at two learning rates (param_ref.ADAM_RANGES),
    from random moments at t = 41 -> 42; the clip of the whole arena before it; then five consecutive steps from zero
    moments, each judged against float64 from the kernel's previous fp32 state."""
    from hp_vae_gan_amd import optim, train
    opt, netG, _ = P.video_nets(1)
    netG.to(DEV)
    arena = optim.ParamArena(netG)
    assert arena.total == P.ARENA_FLOATS["G1"]
    beta1 = float(opt.beta1)
    adam = optim.FlatAdam(arena, train.generator_param_groups(opt, netG), betas=(beta1, HP["beta2"]), eps=HP["eps"])
    ranges = P.ADAM_RANGES["G1"]
    assert [(g["lo"], g["hi"]) for g in adam.groups] == [(lo, hi) for lo, hi, _ in ranges]
    real = torch.zeros(arena.total, dtype=torch.bool, device=DEV)
    for q in arena.params:
        o, cnt = arena.range[id(q)]
        real[o:o + cnt] = True
    assert not bool(real.all())                  # the padding: p = g = m = v = 0, where the update is 0
    g0 = _gen("arena")

    def new_grad(scale):
        arena.grad.copy_(scale * torch.randn(arena.total, generator=g0, device=DEV) * real)

    # clip through the arena
    new_grad(0.01)
    grad = arena.grad.clone()
    info = torch.empty(2, device=DEV)
    arena.clip_grad_norm_(5.0, info)
    (total, tA), (coef, cA) = P.clip64(ops.sqsum(grad), 5.0)
    assert float(coef) < 1
    _check_scalar(info[1], total, tA, "arena clip: total", "clip.total", "arena G1")
    _check_scalar(info[0], coef, cA, "arena clip: coef", "clip.coef", "arena G1")
    _check(arena.grad, *P.clip_apply64(grad, coef), "arena clip: g", "clip.g", "arena G1")

    # one step from random moments, t = 41 -> 42
    for grp in adam.groups:
        grp["m"].copy_(0.01 * torch.randn(grp["m"].shape, generator=g0, device=DEV) * real[grp["lo"]:grp["hi"]])
        grp["v"].copy_((0.01 * torch.randn(grp["v"].shape, generator=g0, device=DEV) * real[grp["lo"]:grp["hi"]]) ** 2)
    adam.t = 41
    adam.t_dev.fill_(41)

    def step_and_check(what):
        before = [(arena.flat[grp["lo"]:grp["hi"]].clone(), arena.grad[grp["lo"]:grp["hi"]].clone(), grp["m"].clone(),
                   grp["v"].clone()) for grp in adam.groups]
        adam.step()
        torch.cuda.synchronize()
        t = adam.steps()
        assert t == adam.t
        for grp, b, (lo, hi, lr) in zip(adam.groups, before, ranges):
            after = (arena.flat[lo:hi], grp["m"], grp["v"])
            _check_adam("%s, t=%d, range [%d, %d) lr %g: " % (what, t, lo, hi, lr), "arena G1 lr=%g" % lr, b, after, t, grp["lr"], beta1)
            pad = ~real[lo:hi]
            assert torch.equal(after[0][pad], b[0][pad]) and float(grp["m"][pad].abs().sum()) == 0.0
        return t

    assert step_and_check("arena step from random moments") == 42

    # five consecutive steps from zero moments
    adam = optim.FlatAdam(arena, train.generator_param_groups(opt, netG), betas=(beta1, HP["beta2"]), eps=HP["eps"])
    for k in range(1, 6):
        new_grad(10.0 ** (k - 4))
        assert step_and_check("arena, consecutive steps") == k
