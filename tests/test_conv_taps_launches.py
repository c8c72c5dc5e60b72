"""Every launch form of the tap-generic conv family (hpvg_convk_fwd_f32, hpvg_convk_bwd_weight_f32) on the GPU, element by
element against the float64 references of tests/conv_taps_ref.py: |got - ref| <= TAU * A with conv_ref.TAU = 1e-5.

Forms: forward plain, forward with bias + LeakyReLU, forward with out_mask, backward-data (flip, with out_mask), weight
gradient fresh and accumulated; K = 5 and 7 in 3-D and 2-D, K = 3 through the same entry points; two identical launches give
the same bits; ops routes 5- and 7-tap weights here; the gradient penalty's double backward through ops.Conv.

Shapes (B, Cin, Cout, T, H, W) are the smallest at which each mechanism can fail.  The kernels' spatial tiles: the forward
kernel covers TH x 32 outputs of one plane per workgroup with TH = 512 // (32 + 2 (K // 2)) = 15 / 14 / 13 for K = 3 / 5 / 7
(FWD_TH below), stages 16 input channels per chunk and 32 or 64 output channels per workgroup; the weight-gradient kernel
walks 4 x 32 position tiles and 64 x 64 channel blocks.  So "one more than the tile" is H = TH + 1 (also 4 + 1 rows and more
for the weight gradient) and W = 33, and 72 channels give five channel chunks, three M tiles (on these few spatial tiles one
per workgroup; two_tile_cases below are the grids that take two per workgroup, the form the default widths run) and four
channel blocks.

The worst ratio per (form, K, dims) is printed at the end of the module and, when HPVG_TAPS_STATS names a file, written
there (profiles/conv_taps_launches.txt is that file from a run on an MI355X)."""
import os

import pytest
import torch

import conv_taps_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
FWD_TH = {3: 15, 5: 14, 7: 13}
_STATS = {}


def cases(K):
    return [
        (1, 5, 7, 1, 1, 1), (2, 3, 16, 2, 3, 4),                          # a volume smaller than the halo on every axis
        (2, 3, 16, 3, 6, 9), (1, 16, 3, 3, 6, 9), (1, 16, 1, 4, 5, 37),   # odd and tiny channel counts, 3 / 1 outputs
        (1, 8, 8, 2, FWD_TH[K] + 1, 33),                                  # one more than the spatial tile along H and W
        (1, 72, 72, K, 9, 11),                                            # channel chunks, M tiles, channel blocks
        (4, 16, 16, K, 9, 11),                                            # the weight gradient's reduce across samples
    ]


def two_tile_cases(K):
    """Launches that run convk_fwd_kernel<K, 2>, the form every default-width (nfc 64) level at the finest sizes takes: Cout > 32
    and more two-tile workgroups than the chip has CUs (B * T * ceil(H / TH) * ceil(W / 32) * ceil(Cout / 64) > 256; the cases above
    have 1 to 7 spatial tiles and run one M tile per workgroup).  2-D: 8 * 9 * 8 = 576 spatial tiles, Cout 72 = two workgroup
    rows, the second with 8 of its 64 channels real, odd Cin; the flipped launch (Cout 5) runs one tile.  3-D: 16 * 16 * 1 * 2 =
    512 tiles of tiny planes, Cout 40 = one row with a partly filled second tile, two channel chunks; flipped: Cout 18."""
    return [(8, 5, 72, 1, 8 * FWD_TH[K] + 1, 225), (16, 18, 40, 16, 2, 33)]


def fwd_tiles(K, case, dims, cout):
    B, _, _, T, H, W = case
    T = T if dims == 3 else 1
    return B * T * -(-H // FWD_TH[K]) * -(-W // 32) * -(-cout // 64)


PARAMS = [(K, dims, c) for K in (5, 7) for dims in (3, 2) for c in cases(K)] + \
         [(K, 2, two_tile_cases(K)[0]) for K in (5, 7)] + [(K, 3, two_tile_cases(K)[1]) for K in (5, 7)] + \
         [(3, dims, c) for dims in (3, 2) for c in (cases(3)[1], cases(3)[4], cases(3)[5], cases(3)[6])]
IDS = ["K%d-%dd-%s" % (K, dims, "x".join(map(str, c))) for K, dims, c in PARAMS]


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    lines = ["worst |got - ref| / A per (form, K, dims), tau %.0e:" % R.TAU]
    for (form, K, dims), (v, case) in sorted(_STATS.items()):
        lines.append("  %-22s K=%d %dd  %.3e  at %s" % (form, K, dims, v, "x".join(map(str, case))))
    print("\n" + "\n".join(lines))
    path = os.environ.get("HPVG_TAPS_STATS")
    if path:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


def fwd(x, w, bias=None, lrelu=False, mask=None, flip=False):
    """hpvg_convk_fwd_f32 as the C ABI has it (any K the library takes, 3 included)."""
    from hp_vae_gan_amd import ops
    from hp_vae_gan_amd.lib import call, ptr, stream
    K = w.shape[2]
    cin, cout = (w.shape[0], w.shape[1]) if flip else (w.shape[1], w.shape[0])
    g = R.geo(x.shape, cin, cout, K)
    y = torch.full((x.shape[0], cout) + tuple(x.shape[2:]), float("nan"), device=x.device)
    ws = ops._scratch(call("hpvg_convk_fwd_ws_bytes", *g), x.device)
    call("hpvg_convk_fwd_f32", ptr(x), ptr(w), ptr(bias), ptr(y), 1 if lrelu else 0, ptr(mask), 1 if flip else 0, *ws, *g, stream())
    return y


def wgrad(dy, x, w_shape, into=None):
    from hp_vae_gan_amd import ops
    from hp_vae_gan_amd.lib import call, ptr, stream
    g = R.geo(x.shape, w_shape[1], w_shape[0], w_shape[2])
    dw = into if into is not None else torch.full(tuple(w_shape), float("nan"), device=x.device)
    ws = ops._scratch(call("hpvg_convk_bwd_weight_ws_bytes", *g), x.device)
    call("hpvg_convk_bwd_weight_f32", ptr(dy), ptr(x), ptr(dw), 1 if into is not None else 0, *ws, *g, stream())
    return dw


def _check(got, ref, A, form, K, dims, case, names=None):
    r = R.check(got, ref, A, "%s K=%d %dd %s" % (form, K, dims, case), names=names)
    key = (form, K, dims)
    if r > _STATS.get(key, (-1.0, None))[0]:
        _STATS[key] = (r, case)


@pytest.mark.parametrize("K,dims,case", PARAMS, ids=IDS)
def test_launches_match_float64(K, dims, case):
    from conv_ref import WEIGHT_NAMES
    from launch_common import fill_workspaces
    from hp_vae_gan_amd import ops
    x, w, b, dy = R.make_case(case, K, dims)
    xd, wd, bd, dyd = (t.to(DEV) for t in (x, w, b, dy))
    if case in two_tile_cases(K):     # the case is here to run the two-M-tile kernel: see that the size rule picks it
        assert case[2] > 32 and fwd_tiles(K, case, dims, case[2]) > 256, fwd_tiles(K, case, dims, case[2])
    y64, A = R.conv_fwd64(x, w)
    # ---- forward: plain, bias + LeakyReLU, out_mask
    y = fwd(xd, wd)
    _check(y, y64, A, "fwd", K, dims, case)
    yb64, Ab = R.conv_fwd64(x, w, b)
    yb = fwd(xd, wd, bias=bd, lrelu=True)
    _check(yb, R.lrelu(yb64), Ab, "fwd bias lrelu", K, dims, case)
    g = torch.Generator().manual_seed(3)
    m = torch.rand(y64.shape, generator=g) - 0.5
    m[m.abs() < 0.05] = 0.0                      # zeros and negatives both take the 0.2 branch
    scale = torch.where(m > 0, 1.0, 0.2).double()
    ym = fwd(xd, wd, bias=bd, mask=m.to(DEV))
    _check(ym, yb64 * scale, Ab, "fwd out_mask", K, dims, case)
    # ---- backward-data: the flipped, transposed weight; with the mask of the activation below
    dx64, Ad = R.conv_bwd_data64(dy, w)
    dx = fwd(dyd, wd, flip=True)
    _check(dx, dx64, Ad, "bwd_data", K, dims, case)
    mx = torch.rand(dx64.shape, generator=g) - 0.5
    dxm = fwd(dyd, wd, flip=True, mask=mx.to(DEV))
    _check(dxm, dx64 * torch.where(mx > 0, 1.0, 0.2).double(), Ad, "bwd_data out_mask", K, dims, case)
    # ---- weight gradient: fresh, accumulated
    dw64, Aw = R.conv_bwd_weight64(dy, x, w.shape)
    dw = wgrad(dyd, xd, w.shape)
    _check(dw, dw64, Aw, "wgrad", K, dims, case, names=WEIGHT_NAMES[dims + 2])
    base = (torch.rand(w.shape, generator=g) - 0.5) * float(Aw.mean())
    acc = wgrad(dyd, xd, w.shape, into=base.to(DEV))
    _check(acc, dw64 + base.double(), Aw + base.abs(), "wgrad accumulate", K, dims, case, names=WEIGHT_NAMES[dims + 2])
    # ---- the same launches again, with every workspace byte 0xFF in between: the same bits
    fill_workspaces(ops)
    assert torch.equal(fwd(xd, wd), y), "fwd: two launches differ"
    fill_workspaces(ops)
    assert torch.equal(fwd(xd, wd, bias=bd, lrelu=True), yb)
    assert torch.equal(fwd(dyd, wd, flip=True), dx), "bwd_data: two launches differ"
    fill_workspaces(ops)
    assert torch.equal(wgrad(dyd, xd, w.shape), dw), "wgrad: two launches differ"
    assert torch.equal(wgrad(dyd, xd, w.shape, into=base.to(DEV)), acc)


@pytest.mark.parametrize("K,dims,case", [(K, 2, two_tile_cases(K)[0]) for K in (5, 7)] + [(5, 3, two_tile_cases(5)[1]), (7, 3, (1, 72, 72, 7, 9, 11))],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_one_and_two_m_tiles_per_workgroup_give_the_same_bits(K, dims, case):
    """hpvg_convk_fwd_mt_config: the launcher takes one or two 32-channel M tiles per workgroup by grid size, and every output's
    sum has the same order in both - so forcing either form (1, 2) must give the bits of the size rule (0), for every forward
    form, on a grid the rule gives two tiles and on one it gives one; and the forced two-tile form meets the float64 bound
    on the small grid too."""
    from hp_vae_gan_amd.lib import load
    lib = load()
    x, w, b, dy = R.make_case(case, K, dims)
    xd, wd, bd, dyd = (t.to(DEV) for t in (x, w, b, dy))
    g = torch.Generator().manual_seed(4)
    m = (torch.rand(dy.shape, generator=g) - 0.5).to(DEV)
    mx = (torch.rand(x.shape, generator=g) - 0.5).to(DEV)

    def forms():
        return [fwd(xd, wd), fwd(xd, wd, bias=bd, lrelu=True), fwd(xd, wd, bias=bd, mask=m), fwd(dyd, wd, flip=True, mask=mx)]

    assert lib.hpvg_convk_fwd_mt_config(-1) == 0
    try:
        by_size = forms()
        assert lib.hpvg_convk_fwd_mt_config(1) == 1
        one = forms()
        assert lib.hpvg_convk_fwd_mt_config(2) == 2
        two = forms()
    finally:
        assert lib.hpvg_convk_fwd_mt_config(0) == 0
    for name, a, o, t in zip(("fwd", "fwd bias lrelu", "fwd out_mask", "bwd_data out_mask"), by_size, one, two):
        assert torch.equal(a, o), "%s: one M tile per workgroup differs from the size rule's launch" % name
        assert torch.equal(a, t), "%s: two M tiles per workgroup differ from the size rule's launch" % name
    y64, A = R.conv_fwd64(x, w)
    _check(two[0], y64, A, "fwd forced 2 tiles", K, dims, case)


@pytest.mark.parametrize("K,dims", [(5, 3), (7, 2)])
def test_ops_routes_wide_weights_to_this_family(K, dims):
    """ops.conv_fwd_raw / conv_bwd_weight_raw decide by the weight's tap side: the bits are those of the raw entry points; no
    1-bit mask is made, no pack is cached, the fused weight + bias gradient launch declines."""
    from hp_vae_gan_amd import ops
    case = (2, 3, 16, 3, 6, 9)
    x, w, b, dy = R.make_case(case, K, dims)
    xd, wd, bd, dyd = (t.to(DEV) for t in (x, w, b, dy))
    ops.weights_changed()
    assert torch.equal(ops.conv_fwd_raw(xd, wd, bd, out_lrelu=True), fwd(xd, wd, bias=bd, lrelu=True))
    y, bits = ops.conv_fwd_raw(xd, wd, bd, out_lrelu=True, want_bits=True)
    assert bits is None and torch.equal(y, fwd(xd, wd, bias=bd, lrelu=True))
    assert torch.equal(ops.conv_fwd_raw(dyd, wd, None, flip=True, out_mask=xd), fwd(dyd, wd, flip=True, mask=xd))
    assert not ops._pack_cache and ops.pack_weight(wd, False) is wd
    ops.prepack_weights([wd, wd])
    assert not ops._pack_cache
    assert torch.equal(ops.conv_bwd_weight_raw(dyd, xd, w.shape), wgrad(dyd, xd, w.shape))
    into = torch.ones(w.shape, device=DEV)
    assert ops.conv_bwd_weight_raw(dyd, xd, w.shape, into=into) is None
    assert torch.equal(into, wgrad(dyd, xd, w.shape, into=torch.ones(w.shape, device=DEV)))
    assert ops.conv_bwd_weight_bias_raw(dyd, xd, w.shape, into, torch.zeros(16, device=DEV)) is False
    seen = []
    ops.set_kernel_timer(ops.KernelTimer(lambda d: seen.append(dict(d)) or None))
    try:
        ops.conv_fwd_raw(xd, wd, None)
        ops.conv_bwd_weight_raw(dyd, xd, w.shape)
    finally:
        ops.set_kernel_timer(None)
    assert [d["K"] for d in seen] == [K, K] and [d["op"] for d in seen] == ["conv", "wgrad"]
    for bad in ((16, 3, 5, 5, 3), (16, 3, 9, 9)):
        with pytest.raises(RuntimeError):
            ops.conv_fwd_raw(xd, torch.zeros(bad, device=DEV), None)


def test_double_backward_through_ops_conv():
    """The gradient penalty's route: torch.autograd.grad(..., create_graph=True) through ops.Conv with a 5-tap weight, then a
    backward of a function of that gradient.  Both second-order products - d/dw and d/dx of <grad_x, v> - against float64
    autograd of F.conv3d, on the error scale of the same products of absolute values."""
    from hp_vae_gan_amd import ops
    import torch.nn.functional as F
    K = 5
    x, w, b, dy = R.make_case((2, 3, 8, 3, 6, 9), K, 3)
    g = torch.Generator().manual_seed(5)
    v = torch.rand(x.shape, generator=g) * 2 - 1
    u = torch.rand(dy.shape, generator=g) * 2 - 1

    def penalty(conv, x, w, b, u, v):
        """L = <d<conv(x), u * conv(x)> / dx, v>: quadratic in the conv's output, so d2/dx dw and d2/dx dx are both non-zero"""
        y = conv(x, w, b)
        (gx,) = torch.autograd.grad(((y * y) * u).sum() * 0.5, x, create_graph=True)
        return (gx * v).sum(), gx

    xr, wr, br = (t.double().requires_grad_(True) for t in (x, w, b))
    L64, gx64 = penalty(lambda a, c, d: F.conv3d(a, c, d, padding=K // 2), xr, wr, br, u.double(), v.double())
    dx64, dw64, db64 = torch.autograd.grad(L64, (xr, wr, br))
    xa, wa, ba = (t.double().abs().requires_grad_(True) for t in (x, w, b))
    La, gxa = penalty(lambda a, c, d: F.conv3d(a, c, d, padding=K // 2), xa, wa, ba, u.double().abs(), v.double().abs())
    dxa, dwa, dba = torch.autograd.grad(La, (xa, wa, ba))

    xd, wd, bd = (t.to(DEV).requires_grad_(True) for t in (x, w, b))
    L, gx = penalty(lambda a, c, d: ops.Conv.apply(a, c, d, False), xd, wd, bd, u.to(DEV), v.to(DEV))
    dx, dw, db = torch.autograd.grad(L, (xd, wd, bd))
    # the same bound as every single launch, TAU on the scale of the absolute-value twin of the whole expression; the worst
    # ratios go to the module's report with the other forms
    case = (2, 3, 8, 3, 6, 9)
    for got, ref, A, form, depth, names in ((gx, gx64.detach(), gxa.detach(), "gp first-order dx", 1, None), (dx, dx64, dxa, "gp second-order d/dx", 1, None),
                                           (dw, dw64, dwa, "gp second-order d/dw", 1, ("o", "i", "kt", "kh", "kw")),
                                           (db, db64, dba, "gp second-order d/db", 1, None)):
        r = R.check(got, ref, A.float(), form, tau=depth * R.TAU, names=names)
        _STATS[(form, K, 3)] = (r, case)
