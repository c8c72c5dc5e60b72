"""Every launch of csrc/variants.hip - Gate, GlobalAvgPool, CodeTimesMap, ReparamBern, KLBern (modules/_nets.py's _nb models) -
element-wise against the float64 references of tests/variant_ref.py: conv_ref.check at ew_ref.TAU with the error scales derived
there.  tests/test_variants.py runs one whole GeneratorVAE_nb at the coarsest level against recorded vectors; here each kernel
is launched on its own, through ops and - where a nullable argument needs it - through the C ABI:

  shapes    the fixture's coarsest levels (3-D and 2-D), S = 1, S = 257 (the row sum's second trip) and B = 2, C = 2,
            S = 300 000: B * S > 2048 * 256 sends every column kernel's grid-stride loop round, n > 1024 * 256 the KL partials';
  gate_bwd  dout only, dbern_ext only, both; df and dlogit null as ops.Gate.backward passes them; logits up to |6|;
  code x map  gradients wanted for the code only, the map only, both;
  edges     x in {0, 1, 2^-24, 1 - 2^-24, 1e-30}, eps in {0, 1 - 2^-24}, forward and backward of reparam_bern and kl_bern: the
            float64 reference is finite at all of them, so the kernel's result must be;
  workspace the KL forward once more after launch_common.fill_workspaces, bit for bit.
The launches at 4-byte offsets are section (c) of tests/test_offset_launches.py.  The module prints the worst |got - ref| / A per
quantity and shape class."""
import zlib

import pytest
import torch

import launch_common as LC
import offset_buf as OB
import variant_ref as V

pytestmark = pytest.mark.gpu

DEV = "cuda"
_STATS = {}
_COUNT = {"launches": 0, "f64": 0}

# (B, C, spatial): the variants fixture's coarsest levels, S = 1, S = 257, and the grid-stride shape
SHAPES = [(2, 8, (4, 12, 16)), (2, 8, (12, 16)), (3, 5, (1, 1, 1)), (2, 3, (257,)), (2, 2, (3, 100, 1000))]
IDS = ["fixture3d", "fixture2d", "S1", "S257", "gridstride"]


@pytest.fixture(scope="module")
def ops():
    import hp_vae_gan_amd  # noqa: F401
    from hp_vae_gan_amd import ops as _ops
    yield _ops
    print("\nvariants: %d launches, %d quantities compared with float64" % (_COUNT["launches"], _COUNT["f64"]))
    LC.print_stats(_STATS, "    worst |got - ref| / A per (quantity, shape), tau %.0e:" % V.TAU)


@pytest.fixture(scope="module")
def hplib(ops):
    from hp_vae_gan_amd import lib as _hplib
    _hplib.load()
    return _hplib


def _gen(*key):
    return torch.Generator(device=DEV).manual_seed(zlib.crc32(repr(key).encode()))


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, device=DEV)


def _leaf(t):
    return t.detach().clone().requires_grad_(True)


def _S(sp):
    n = 1
    for v in sp:
        n *= v
    return n


def check(got, ref, A, what, quantity, key, launches=1):
    LC.checked(_STATS, got.reshape(ref.shape), ref, A, what, quantity, key, tau=V.TAU)
    _COUNT["f64"] += 1
    _COUNT["launches"] += launches


def _logits(g, B, S):
    """N(0, 3^2) clamped to [-6, 6], with both ends present: 1 - sigmoid(6) = 2.5e-3."""
    l = (3 * _randn(g, B, S)).clamp_(-6, 6)
    l.view(-1)[0] = 6.0
    l.view(-1)[-1] = -6.0
    return l


# ------------------------------------------------------------------------------------------------ through ops
@pytest.mark.parametrize("B,C,sp", SHAPES, ids=IDS)
def test_variant_launches_through_ops(ops, B, C, sp, request):
    key = request.node.callspec.id
    S = _S(sp)
    if key == "gridstride":
        assert B * S > 2048 * 256 and B * C * S > 2048 * 256
    g = _gen("ops", B, C, sp)
    f, dout, dz = (_randn(g, B, C, *sp) for _ in range(3))
    logit, dbern, zmap = _logits(g, B, S).view(B, 1, *sp), _randn(g, B, 1, *sp), _randn(g, B, 1, *sp)
    one = (1,) * len(sp)
    code, gpool = _randn(g, B, C, *one), _randn(g, B, C, *one)
    f3, dout3, dz3 = f.view(B, C, S), dout.view(B, C, S), dz.view(B, C, S)
    tag = "%s B=%d C=%d %s: " % (key, B, C, sp)

    # Gate: forward, then the backward with both incoming gradients
    fl, ll = _leaf(f), _leaf(logit)
    out, bern = ops.Gate.apply(fl, ll)
    ref = V.gate_fwd64(f3, logit.view(B, S))
    check(out.detach().view(B, C, S), *ref["out"], tag + "gate out", "gate.out", key)
    check(bern.detach().view(B, S), *ref["bern"], tag + "gate bern", "gate.bern", key, 0)
    df, dlogit = torch.autograd.grad([out, bern], [fl, ll], [dout, dbern])
    bref = V.gate_bwd64(dout3, f3, bern.detach().view(B, S), dbern.view(B, S))
    check(df.view(B, C, S), *bref["df"], tag + "gate df", "gate.df", key)
    check(dlogit.view(B, S), *bref["dlogit"], tag + "gate dlogit", "gate.dlogit", key, 0)

    # GlobalAvgPool
    xl = _leaf(f)
    pooled = ops.GlobalAvgPool.apply(xl)
    assert tuple(pooled.shape) == (B, C) + one
    check(pooled.detach().view(B, C), *V.pool_fwd64(f3), tag + "pool", "pool.fwd", key)
    (dx,) = torch.autograd.grad(pooled, [xl], gpool)
    check(dx.view(B, C, S), *V.pool_bwd64(gpool.view(B, C), S), tag + "pool backward", "pool.bwd", key)

    # CodeTimesMap
    cl, ml = _leaf(code), _leaf(zmap)
    z = ops.CodeTimesMap.apply(cl, ml)
    assert tuple(z.shape) == (B, C) + tuple(sp)
    check(z.detach().view(B, C, S), *V.outer64(code.view(B, C), zmap.view(B, S), 1.0, S), tag + "code x map", "codemap.fwd", key)
    dcode, dmap = torch.autograd.grad(z, [cl, ml], dz)
    check(dcode.view(B, C), *V.rowsum64(dz3, zmap.view(B, S), 1.0), tag + "dcode", "codemap.dcode", key)
    check(dmap.view(B, S), *V.colsum64(dz3, code.view(B, C)), tag + "dmap", "codemap.dmap", key)

    # ReparamBern and KLBern on [B, 1, sp] maps in (0, 1)
    n = B * S
    x = torch.rand(B, 1, *sp, generator=g, device=DEV) * 0.98 + 0.01
    eps = torch.rand(B, 1, *sp, generator=g, device=DEV)
    if key == "gridstride":
        x = x.expand(B, 2, *sp).contiguous()              # n = 1.2M: past 1024 * 256 partial blocks' first trip, and past 2048 * 256
        eps = eps.expand(B, 2, *sp).contiguous()
        n = x.numel()
        assert n > 2048 * 256
    dzb = _randn(g, *x.shape)
    xl = _leaf(x)
    zb = ops.ReparamBern.apply(xl, eps)
    check(zb.detach().view(-1), *V.reparam_bern_fwd64(x.view(-1), eps.view(-1)), tag + "reparam_bern", "rbern.fwd", key)
    (dxb,) = torch.autograd.grad(zb, [xl], dzb)
    check(dxb.view(-1), *V.reparam_bern_bwd64(dzb.view(-1), x.view(-1)), tag + "reparam_bern backward", "rbern.bwd", key)
    xl = _leaf(x)
    kl = ops.KLBern.apply(xl)
    r, A = V.kl_bern_fwd64(x)
    check(kl.detach().reshape(1), r.reshape(1), A.reshape(1), tag + "kl_bern", "klbern.fwd", key)
    gout = torch.tensor(0.83, device=DEV)
    (dxk,) = torch.autograd.grad(kl, [xl], gout)
    check(dxk.view(-1), *V.kl_bern_bwd64(0.83, x.view(-1)), tag + "kl_bern backward", "klbern.bwd", key)

    # the KL forward on a poisoned workspace: bit for bit
    LC.fill_workspaces(ops)
    again = ops.KLBern.apply(x)
    torch.cuda.synchronize()
    assert torch.equal(again.detach().reshape(1), kl.detach().reshape(1)), tag + "kl_bern differs after the workspace was filled with 0xFF"
    _COUNT["launches"] += 1


# ------------------------------------------------------------------------------------------------ nullable arguments
GATE_SHAPES = [(2, 8, 768), (3, 5, 1), (2, 3, 257)]


@pytest.mark.parametrize("B,C,S", GATE_SHAPES, ids=["fixture3d", "S1", "S257"])
def test_gate_bwd_nullable_arguments_through_the_c_abi(ops, hplib, B, C, S, request):
    """hpvg_gate_bwd_f32 with dout only, dbern_ext only and both, each with (df, dlogit), df alone and dlogit alone, into
    guarded outputs; a null output's companion is unchanged by its absence (bit-equal to the launch that has both)."""
    key = request.node.callspec.id
    g = _gen("gate_bwd", B, C, S)
    f, dout, ext = _randn(g, B, C, S), _randn(g, B, C, S), _randn(g, B, S)
    logit = _logits(g, B, S)
    out, bern = torch.empty_like(f), torch.empty_like(logit)
    p = hplib.ptr
    hplib.call("hpvg_gate_fwd_f32", p(f), p(logit), p(out), p(bern), B, C, S, hplib.stream())
    f32 = torch.float32
    for dname, d, e in (("dout", dout, None), ("dbern_ext", None, ext), ("both", dout, ext)):
        bref = V.gate_bwd64(d, f, bern, e)
        full = None
        for want_df, want_dl in ((True, True), (True, False), (False, True)):
            df = OB.out_like((B, C, S), f32, 0, device=DEV) if want_df else None
            dl = OB.out_like((B, S), f32, 0, device=DEV) if want_dl else None
            hplib.call("hpvg_gate_bwd_f32", p(d), p(f), p(bern), p(e), p(df), p(dl), B, C, S, hplib.stream())
            torch.cuda.synchronize()
            tag = "gate_bwd %s B=%d C=%d S=%d, %s: " % (key, B, C, S, dname) + ("df " if want_df else "") + ("dlogit" if want_dl else "")
            if want_df:
                OB.assert_written(df, tag + " df")
                check(df, *bref["df"], tag, "gate.df." + dname, key)
            if want_dl:
                OB.assert_written(dl, tag + " dlogit")
                check(dl, *bref["dlogit"], tag, "gate.dlogit." + dname, key, 0 if want_df else 1)
            if full is None:
                full = (df.clone(), dl.clone())
            else:
                assert df is None or torch.equal(df, full[0]), tag + ": df depends on dlogit being asked for"
                assert dl is None or torch.equal(dl, full[1]), tag + ": dlogit depends on df being asked for"
    # without dout, df is 0 * bern = 0 everywhere
    assert not bool(V.gate_bwd64(None, f, bern, ext)["df"][0].any())
    # neither gradient: refused
    assert hplib.load().hpvg_gate_bwd_f32(None, p(f), p(bern), None, p(out), p(bern.clone()), B, C, S, hplib.stream()) != 0


@pytest.mark.parametrize("B,C,S", GATE_SHAPES, ids=["fixture3d", "S1", "S257"])
def test_needs_input_grad_combinations(ops, B, C, S, request):
    """ops.Gate.backward and ops.CodeTimesMap.backward with a gradient wanted for one input only (the other launch, or the other
    output pointer, is left out) and with only one of the gate's two outputs used."""
    key = request.node.callspec.id
    g = _gen("needs", B, C, S)
    f, dout, dz = (_randn(g, B, C, S) for _ in range(3))
    logit, dbern, zmap = _logits(g, B, S).view(B, 1, S), _randn(g, B, 1, S), _randn(g, B, 1, S)
    code = _randn(g, B, C, 1)
    tag = "%s B=%d C=%d S=%d: " % (key, B, C, S)

    def gate(f_grad, l_grad, use_out, use_bern):
        fl = _leaf(f) if f_grad else f
        ll = _leaf(logit) if l_grad else logit
        out, bern = ops.Gate.apply(fl, ll)
        outs = ([out] if use_out else []) + ([bern] if use_bern else [])
        gs = ([dout] if use_out else []) + ([dbern] if use_bern else [])
        ins = ([fl] if f_grad else []) + ([ll] if l_grad else [])
        grads = list(torch.autograd.grad(outs, ins, gs, allow_unused=True))
        bref = V.gate_bwd64(dout if use_out else None, f, bern.detach().view(B, S), dbern.view(B, S) if use_bern else None)
        if f_grad:
            df = grads.pop(0)
            if use_out:
                check(df, *bref["df"], tag + "gate df (f_grad=%s l_grad=%s)" % (f_grad, l_grad), "gate.df.ops", key)
            else:
                assert df is None or not bool(df.any()), tag + "df without dout must be absent or zero"
        if l_grad:
            check(grads.pop(0).view(B, S), *bref["dlogit"], tag + "gate dlogit (out=%s bern=%s)" % (use_out, use_bern),
                  "gate.dlogit.ops", key, 0 if f_grad and use_out else 1)

    for f_grad, l_grad in ((True, False), (False, True), (True, True)):
        for use_out, use_bern in ((True, False), (False, True), (True, True)):
            if not use_out and not l_grad:
                continue                                   # bern does not depend on f: autograd has nothing to run
            gate(f_grad, l_grad, use_out, use_bern)

    for c_grad, m_grad in ((True, False), (False, True), (True, True)):
        cl = _leaf(code) if c_grad else code
        ml = _leaf(zmap) if m_grad else zmap
        z = ops.CodeTimesMap.apply(cl, ml)
        grads = list(torch.autograd.grad(z, ([cl] if c_grad else []) + ([ml] if m_grad else []), dz))
        if c_grad:
            check(grads.pop(0).view(B, C), *V.rowsum64(dz, zmap.view(B, S), 1.0), tag + "dcode (map grad %s)" % m_grad,
                  "codemap.dcode.ops", key)
        if m_grad:
            check(grads.pop(0).view(B, S), *V.colsum64(dz, code.view(B, C)), tag + "dmap (code grad %s)" % c_grad,
                  "codemap.dmap.ops", key)


# ------------------------------------------------------------------------------------------------ the + 1e-20 edges
def test_bernoulli_edges_forward_and_backward(ops):
    g = _gen("edges")
    n = 1500
    x, eps = V.edge_inputs(n, g, device=DEV)
    ne = len(V.X_EDGES) * len(V.EPS_EDGES)
    pairs = {(float(a), float(b)) for a, b in zip(x[:ne].cpu(), eps[:ne].cpu())}
    assert len(pairs) == ne and {a for a, _ in pairs} == {float(torch.tensor(v, dtype=torch.float32)) for v in V.X_EDGES}
    dz = _randn(g, n)
    xl = _leaf(x)
    z = ops.ReparamBern.apply(xl, eps)
    ref, A = V.reparam_bern_fwd64(x, eps)
    assert bool(torch.isfinite(ref).all())
    assert bool(torch.isfinite(z).all()), "reparam_bern is not finite at %s" % (x[~torch.isfinite(z)].tolist(),)
    check(z.detach(), ref, A, "reparam_bern at the edges", "rbern.fwd", "edges")
    (dx,) = torch.autograd.grad(z, [xl], dz)
    ref, A = V.reparam_bern_bwd64(dz, x)
    assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(dx).all())
    check(dx, ref, A, "reparam_bern backward at the edges", "rbern.bwd", "edges")
    xl = _leaf(x)
    kl = ops.KLBern.apply(xl)
    ref, A = V.kl_bern_fwd64(x)
    assert bool(torch.isfinite(ref)) and bool(torch.isfinite(kl))
    check(kl.detach().reshape(1), ref.reshape(1), A.reshape(1), "kl_bern at the edges", "klbern.fwd", "edges")
    (dxk,) = torch.autograd.grad(kl, [xl], torch.tensor(0.83, device=DEV))
    ref, A = V.kl_bern_bwd64(0.83, x)
    assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(dxk).all())
    check(dxk, ref, A, "kl_bern backward at the edges", "klbern.bwd", "edges")
    # every edge on its own, as the only content of the tensor: the mean is that element's term
    for xe in V.X_EDGES:
        one = torch.full((1,), xe, device=DEV)
        kl1 = ops.KLBern.apply(one)
        ref, A = V.kl_bern_fwd64(one)
        assert bool(torch.isfinite(kl1))
        check(kl1.reshape(1), ref.reshape(1), A.reshape(1), "kl_bern of x = %g alone" % xe, "klbern.fwd", "edges")
