"""Float64 references of the conv family with a per-element error bound, and the list of conv launches the benchmark's
pyramids make (tests/test_conv_launch_host.py, tests/test_conv_launches.py).

Error bound.  The rounding error of a fp32 kernel that sums the products of a conv, in whatever order, scales with the sum
of the products' MAGNITUDES, not with the result.  So every reference below comes with its absolute-value twin A: the same
operation on |x|, |w| and |dy|, the natural error scale of each output element.  `check` then requires
|got_i - ref_i| <= tau * A_i for every element.  The global-maximum measure of helpers.assert_close (RTOL = 1e-3 of
max |ref|) lets a kernel be 1 % wrong in one weight tap; this one does not (test_conv_launch_host.py shows both).

Memory.  The references loop over batch samples: torch's CPU conv in float64 builds an im2col buffer of ~6.6 GB for one
sample at the finest video level (64 channels, 13 x 144 x 256), and the B = 4 reference of that level stays near 10 GB.
Values are kept in float64; the scales A in float32 (a scale, rounded by 6e-8 of itself)."""
import itertools
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# |got - ref| <= TAU * A per element: ~100x the error of a fp32 direct conv (1.1e-7 measured at 2 x 64 x 5 x 45 x 81), and
# 8x below what a 1 % error in a single weight tap produces there (7.9e-5)
TAU = 1e-5

# (Cin, Cout) of the layers at every pyramid level: generator / critic head, body and tails (modules/_nets.py)
LAYERS = ((3, 64), (64, 64), (64, 3), (64, 1))
# the encoder's mu / logvar conv and the decoder's head, which only run at level 0
CODEC_LAYERS = ((64, 128), (128, 64))
# batch sizes of the launches: 2 = one generator pass, 4 = the merged (rec + rand) generator pass, 1 = a batch-split rank
BATCHES = (1, 2, 4)
# the order in which a test walks the batch sizes of one (level, layer): the weight's pack is made by the first launch
# (B = 2, without the two-axis section below stage 7) and then serves launches with and without it, as in training
BATCH_ORDER = (2, 4, 1)
# every layer whose kernel kind the host test pins (LAYERS + CODEC_LAYERS), in the column order of KINDS
KIND_LAYERS = ((3, 64), (64, 64), (64, 3), (64, 1), (128, 64), (64, 128))


def _conv(x, w):
    return F.conv3d(x, w, padding=1) if x.dim() == 5 else F.conv2d(x, w, padding=1)


def _conv_input(shape, w, dy):
    g = torch.nn.grad.conv3d_input if dy.dim() == 5 else torch.nn.grad.conv2d_input
    return g(shape, w, dy, padding=1)


def _conv_weight(x, w_shape, dy):
    g = torch.nn.grad.conv3d_weight if dy.dim() == 5 else torch.nn.grad.conv2d_weight
    return g(x, w_shape, dy, padding=1)


def conv_fwd64(x, w, b=None):
    """y = conv(x, w) + b (zero padding 1, as oracle.hpvg_oracle.conv) in float64 -> (y, A)."""
    w64 = w.detach().double().cpu()
    wa = w64.abs()
    B, sp = x.shape[0], tuple(x.shape[2:])
    y = torch.empty((B, w.shape[0]) + sp, dtype=torch.float64)
    A = torch.empty((B, w.shape[0]) + sp, dtype=torch.float32)
    for i in range(B):
        xi = x[i:i + 1].detach().double().cpu()
        y[i] = _conv(xi, w64)[0]
        A[i] = _conv(xi.abs(), wa)[0]
    if b is not None:
        b64 = b.detach().double().cpu().view(1, -1, *([1] * len(sp)))
        y += b64
        A += b64.abs().float()
    return y, A


def conv_bwd_data64(dy, w):
    """dx = conv_input(dy, w): the backward-data conv of the layer weight w, in float64 -> (dx, A)."""
    w64 = w.detach().double().cpu()
    wa = w64.abs()
    B, sp = dy.shape[0], tuple(dy.shape[2:])
    shape1 = (1, w.shape[1]) + sp
    dx = torch.empty((B, w.shape[1]) + sp, dtype=torch.float64)
    A = torch.empty((B, w.shape[1]) + sp, dtype=torch.float32)
    for i in range(B):
        di = dy[i:i + 1].detach().double().cpu()
        dx[i] = _conv_input(shape1, w64, di)[0]
        A[i] = _conv_input(shape1, wa, di.abs())[0]
    return dx, A


def conv_bwd_weight64(dy, x, w_shape, prefixes=None):
    """dw = conv_weight(x, dy) in float64 -> (dw, A); prefixes (batch counts n): {n: (dw, A) of the first n samples}."""
    B = dy.shape[0]
    want = sorted(set(prefixes)) if prefixes is not None else [B]
    acc = torch.zeros(tuple(w_shape), dtype=torch.float64)
    acca = torch.zeros(tuple(w_shape), dtype=torch.float64)
    out = {}
    for i in range(max(want)):
        di, xi = dy[i:i + 1].detach().double().cpu(), x[i:i + 1].detach().double().cpu()
        acc += _conv_weight(xi, tuple(w_shape), di)
        acca += _conv_weight(xi.abs(), tuple(w_shape), di.abs())
        if i + 1 in want:
            out[i + 1] = (acc.clone(), acca.float())
    return out if prefixes is not None else out[B]


def bias_sum64(dy, prefixes=None):
    """db[c] = sum over samples and positions of dy[:, c] in float64 -> (db, A); prefixes as in conv_bwd_weight64."""
    d = dy.detach().double().cpu()
    per = d.flatten(2).sum(2)
    pera = d.abs().flatten(2).sum(2)
    want = sorted(set(prefixes)) if prefixes is not None else [dy.shape[0]]
    out = {n: (per[:n].sum(0), pera[:n].sum(0).float()) for n in want}
    return out if prefixes is not None else out[dy.shape[0]]


# ---------------------------------------------------------------------------- the same references as plain sums over taps
# For the baselines' padded volumes (64 channels at 27 x 158 x 270) the im2col of the functions above needs ~16 GB per sample
# and minutes of CPU time per launch.  The functions below state the same three operations as a sum over the 27 (or 9) taps of
# a channel matmul on shifted views of the zero-padded input, in float64 on whatever device the inputs live on (torch's own
# matmul: no code of libhpvg, no MIOpen).  tests/test_baseline_launch_host.py pins them against the functions above.
def _taps(nd):
    return itertools.product(range(3), repeat=nd)


def _pad1(t):
    return F.pad(t, (1, 1) * (t.dim() - 2))


def _shifted(tp, k, sp):
    """[B, C, S] copy of the view of tp (padded by 1) that starts at offset k: element pos is tp[pos + k] = t[pos + k - 1]."""
    v = tp[(slice(None), slice(None)) + tuple(slice(a, a + n) for a, n in zip(k, sp))]
    return v.reshape(tp.shape[0], tp.shape[1], -1)


def _tap(w, k):
    return w[(slice(None), slice(None)) + tuple(k)]


def _fwd_taps(x64, w64):
    sp = tuple(x64.shape[2:])
    xp = _pad1(x64)
    y = torch.zeros(x64.shape[0], w64.shape[0], x64[0, 0].numel(), dtype=torch.float64, device=x64.device)
    for k in _taps(len(sp)):
        y += torch.einsum("oc,bcs->bos", _tap(w64, k), _shifted(xp, k, sp))
    return y.reshape((x64.shape[0], w64.shape[0]) + sp)


def _bwd_data_taps(dy64, w64):
    sp = tuple(dy64.shape[2:])
    dp = _pad1(dy64)
    dx = torch.zeros(dy64.shape[0], w64.shape[1], dy64[0, 0].numel(), dtype=torch.float64, device=dy64.device)
    for k in _taps(len(sp)):
        # y[pos] takes w[k] x[pos + k - 1], so x[q] gives w[k] to y[q - k + 1]: dy's view at offset 2 - k
        dx += torch.einsum("oc,bos->bcs", _tap(w64, k), _shifted(dp, tuple(2 - a for a in k), sp))
    return dx.reshape((dy64.shape[0], w64.shape[1]) + sp)


def _bwd_weight_taps(dy64, x64):
    sp = tuple(dy64.shape[2:])
    xp = _pad1(x64)
    d = dy64.reshape(dy64.shape[0], dy64.shape[1], -1)
    dw = torch.empty((dy64.shape[1], x64.shape[1]) + (3,) * len(sp), dtype=torch.float64, device=dy64.device)
    for k in _taps(len(sp)):
        dw[(slice(None), slice(None)) + tuple(k)] = torch.einsum("bos,bcs->oc", d, _shifted(xp, k, sp))
    return dw


def conv_fwd64_taps(x, w, b=None):
    """conv_fwd64 as a sum over taps, on x's device -> (y, A) (A in float32)."""
    x64, w64 = x.detach().double(), w.detach().double().to(x.device)
    y = _fwd_taps(x64, w64)
    A = _fwd_taps(x64.abs(), w64.abs())
    if b is not None:
        b64 = b.detach().double().to(x.device).view(1, -1, *([1] * (x.dim() - 2)))
        y += b64
        A += b64.abs()
    return y, A.float()


def conv_bwd_data64_taps(dy, w):
    """conv_bwd_data64 as a sum over taps, on dy's device -> (dx, A)."""
    d64, w64 = dy.detach().double(), w.detach().double().to(dy.device)
    return _bwd_data_taps(d64, w64), _bwd_data_taps(d64.abs(), w64.abs()).float()


def conv_bwd_weight64_taps(dy, x):
    """conv_bwd_weight64 (all samples) as one matmul over samples and positions per tap, on dy's device -> (dw, A)."""
    d64, x64 = dy.detach().double(), x.detach().double()
    return _bwd_weight_taps(d64, x64), _bwd_weight_taps(d64.abs(), x64.abs()).float()


def bias_sum64_on(dy):
    """bias_sum64 (all samples) on dy's device -> (db, A)."""
    d = dy.detach().double().flatten(2)
    return d.sum(dim=(0, 2)), d.abs().sum(dim=(0, 2)).float()


def lrelu(t, slope=0.2):
    return torch.where(t > 0, t, slope * t)


_NAMES = {5: ("n", "c", "t", "h", "w"), 4: ("n", "c", "h", "w"), 1: ("c",)}
WEIGHT_NAMES = {5: ("o", "i", "kt", "kh", "kw"), 4: ("o", "i", "kh", "kw")}


def err_ratio(got, ref, A):
    """(max_i |got_i - ref_i| / A_i, index of that element); A_i = 0 admits only an exact result, NaN counts as infinite.
    Computed on the device of ref (float64 references may live on the GPU)."""
    got = got.detach().to(ref.device)
    A = A.to(ref.device)
    assert tuple(got.shape) == tuple(ref.shape) == tuple(A.shape), (tuple(got.shape), tuple(ref.shape), tuple(A.shape))
    rows = got.shape[0] if got.dim() > 1 else 1
    g2, r2, a2 = (t.reshape(rows, -1) for t in (got, ref, A))
    worst, where = -1.0, (0, 0)
    for i in range(rows):
        d = (g2[i].double() - r2[i].double()).abs()
        a = a2[i].double()
        ratio = torch.where(a > 0, d / a, torch.where(d > 0, torch.full_like(d, float("inf")), torch.zeros_like(d)))
        ratio = torch.nan_to_num(ratio, nan=float("inf"))
        j = int(torch.argmax(ratio))
        r = float(ratio[j])
        if r > worst:
            worst, where = r, (i, j)
    i, j = where
    idx = (i,) + tuple(int(v) for v in torch.unravel_index(torch.tensor(j), tuple(got.shape[1:]))) if got.dim() > 1 else (j,)
    return worst, idx


def check(got, ref, A, what, tau=TAU, names=None):
    """Every element within tau * A_i of the float64 reference, and the plain RTOL check of the suite beside it.  Returns
    the worst ratio |got - ref| / A; on failure the message names the worst element, e.g. (n, c, t, h, w)."""
    from helpers import RTOL, assert_close
    worst, idx = err_ratio(got, ref, A)
    if not worst <= tau:
        names = names or _NAMES.get(got.dim(), tuple("d%d" % k for k in range(got.dim())))
        at = ", ".join("%s=%d" % (n, v) for n, v in zip(names, idx))
        g = float(got.detach()[idx])
        raise AssertionError("%s: |got - ref| / A = %.3e > tau %.1e at (%s): got %.9g, ref %.9g, A %.6g" % (
            what, worst, tau, at, g, float(ref[idx]), float(A[idx])))
    assert_close(got, ref, RTOL, what)
    return worst


# ------------------------------------------------------------------------------------------------ the benchmark's launches
def level_shapes():
    """{config: [level shape]} of the benchmark's pyramids, from bench.py's own geometry: video = BASELINE configs[2]
    ([T, H, W]), video8 = configs[3] (--min-size 48), image = configs[1] ([H, W], 2-D convs)."""
    import bench
    opts = {"video": bench._video_opt("cpu"), "video8": bench._video_opt("cpu", min_size=48), "image": bench.image_opt("cpu")}
    return {k: [tuple(int(v) for v in s) for s in bench.stage_shapes(o, bench._HipGeom)] for k, o in opts.items()}


def launch_groups():
    """[(config, level, (Cin, Cout), shape)] in test order: every level shape with LAYERS, the level-0 shapes also with
    CODEC_LAYERS; a (layer, shape) that an earlier config already has (video8's finest level is video's) is left out.
    Each group is launched at every batch size of BATCH_ORDER."""
    seen, out = set(), []
    for cfg, shapes in level_shapes().items():
        for lvl, sp in enumerate(shapes):
            for layer in LAYERS + (CODEC_LAYERS if lvl == 0 else ()):
                key = (layer, sp)
                if key in seen:
                    continue
                seen.add(key)
                out.append((cfg, lvl, layer, sp))
    return out


def kernel_view(sp):
    """(T, H, W, KT) of a level shape as the library's host queries take it (2-D: T = 1, KT = 1)."""
    return (sp[0], sp[1], sp[2], 3) if len(sp) == 3 else (1, sp[0], sp[1], 1)


def kinds_of(lib, B, layer, sp):
    """(forward, backward-data, weight-gradient kind, fuses_bias) the library picks for a launch of this layer."""
    Ci, Co = layer
    T, H, W, KT = kernel_view(sp)
    return (lib.hpvg_conv_fwd_kernel_kind(B, Ci, Co, T, H, W, KT), lib.hpvg_conv_fwd_kernel_kind(B, Co, Ci, T, H, W, KT),
            lib.hpvg_conv_bwd_weight_kernel_kind(B, Ci, Co, T, H, W, KT), lib.hpvg_conv_bwd_weight_fuses_bias(B, Ci, Co, T, H, W, KT))


# Expected kernel kinds at every level shape, for B = 1, 2, 4: one string per batch size, "f... d... w... b..." with one digit
# per layer of KIND_LAYERS (3->64, 64->64, 64->3, 64->1, 128->64, 64->128).  f = forward kind, d = backward-data kind (the
# conv with Cin, Cout swapped), both hpvg_conv_fwd_kernel_kind: 0 direct, 1 one-axis Winograd, 2 two-axis Winograd,
# 3 narrow output.  w = hpvg_conv_bwd_weight_kernel_kind: 2 one-axis Winograd, 3 two-axis Winograd, 4 narrow.
# b = hpvg_conv_bwd_weight_fuses_bias.  A change of the size rules must change this table on purpose: it decides which
# kernel each launch of tests/test_conv_launches.py exercises.
_K1 = "f013311 d310011 w424422 b010011"      # one-axis everywhere
_K1W = "f013311 d310011 w424433 b010011"     # ... the wide weight gradients two-axis
_K12 = "f013312 d310021 w424433 b010011"     # ... and the 64->128 forward / 128->64 backward-data two-axis
_K12W = "f013312 d310021 w434433 b010011"    # ... and the 64->64 weight gradient two-axis
_K21 = "f023321 d320012 w434433 b010011"     # 64->64 two-axis, 64->128 one-axis
_K2 = "f023322 d320022 w434433 b010011"      # two-axis wherever it runs
_I0 = "f003300 d300000 w424422 b010011"      # 2-D: direct
_I1 = "f013311 d310011 w424422 b010011"      # 2-D: one-axis
_I1W = "f013311 d310011 w424433 b010011"
_I1WW = "f013311 d310011 w434433 b010011"
KINDS = {
    # video (configs[2])
    (4, 18, 33): (_K1, _K1, _K1W), (4, 23, 41): (_K1, _K1, _K12), (4, 28, 51): (_K1, _K1W, _K12W),
    (5, 36, 65): (_K1W, _K12W, _K2), (5, 45, 81): (_K12W, _K21, _K12W), (5, 57, 102): (_K12W, _K2, _K2),
    (7, 72, 129): (_K12W, _K2, _K2), (7, 91, 162): (_K2, _K2, _K2), (7, 114, 204): (_K2, _K2, _K2),
    (13, 144, 256): (_K2, _K2, _K2),
    # video8 (configs[3]); its finest level is video's
    (4, 27, 48): (_K1, _K1W, _K12W), (4, 34, 61): (_K1, _K12, _K21), (4, 43, 78): (_K1W, _K12W, _K2),
    (5, 55, 99): (_K12W, _K2, _K2), (5, 70, 125): (_K2, _K2, _K2), (7, 89, 159): (_K2, _K2, _K2),
    (7, 113, 202): (_K2, _K2, _K2),
    # image (configs[1], 2-D)
    (24, 33): (_I0, _I0, _I0), (30, 41): (_I0, _I0, _I0), (38, 51): (_I0, _I0, _I0), (48, 65): (_I0, _I0, _I0),
    (60, 81): (_I0, _I0, _I0), (76, 102): (_I0, _I0, _I1), (96, 129): (_I0, _I1, _I1), (121, 162): (_I0, _I1, _I1W),
    (153, 204): (_I1, _I1W, _I1WW), (192, 256): (_I1, _I1W, _I1WW),
}


def expected_kinds(B, layer, sp):
    """(forward, backward-data, weight-gradient kind, fuses_bias) of KINDS for one launch."""
    s = {p[0]: p[1:] for p in KINDS[tuple(sp)][BATCHES.index(B)].split()}
    j = KIND_LAYERS.index(tuple(layer))
    return int(s["f"][j]), int(s["d"][j]), int(s["w"][j]), int(s["b"][j])


# ------------------------------------------------------------------------------------------------ the baselines' launches
# The SinGAN-3D baselines (bench.py --config baseline, BASELINE configs[4]; the train_video_baselines program) run VALID
# convolutions as a padding-1 conv plus a crop on volumes padded by num_layer + 2 (GeneratorSG, WDiscriminatorBaselines) or
# num_layer (GeneratorCSG; its head and tail: 1) voxels per side (modules/_nets.py), so their launches are at none of the
# level shapes above.  All of them are B = 2: the baseline trainers never merge passes, and the multi-GPU form is a stage
# pipeline.
BASELINE_NETS = ("GeneratorSG", "GeneratorCSG", "WDiscriminatorBaselines")


def baseline_opt(device="cpu", **kw):
    """(opt, level shapes): bench.py's option set of the baseline config (bench.video_opt under CONFIG = "baseline", kw on
    top) with stop_scale set, and its level shapes."""
    import bench
    keep = bench.CONFIG
    bench.CONFIG = "baseline"
    try:
        opt = bench.video_opt(device, **kw)
    finally:
        bench.CONFIG = keep
    shapes = [tuple(int(v) for v in s) for s in bench.stage_shapes(opt, bench._HipGeom)]
    return opt, shapes


def baseline_level_shapes():
    """Level shapes of the baseline config from bench.py's own geometry; they are video8's."""
    _, shapes = baseline_opt()
    assert shapes == level_shapes()["video8"], shapes
    return shapes


def grown(sp, k):
    return tuple(int(v) + k for v in sp)


def baseline_net_groups(net, lvl, opt=None, shapes=None):
    """[((Cin, Cout), shape)] of the conv launches of pyramid level `lvl` of one baselines network, in forward order (the
    num_layer equal convs of the critic once), with the pads as modules/_nets.py computes them from opt.num_layer."""
    if opt is None:
        opt, shapes = baseline_opt()
    sp, n, N, nc = shapes[lvl], int(opt.num_layer), int(opt.nfc), int(opt.nc_im)
    if net == "GeneratorSG":
        # pad = num_layer + 2; head at the padded size, every conv (padding 1 + crop) sheds one voxel per side
        full = 2 * (n + 2)
        return [((nc, N), grown(sp, full))] + [((N, N), grown(sp, full - 2 * (i + 1))) for i in range(n)] + \
               [((N, nc), grown(sp, full - 2 * (n + 1)))]
    if net == "GeneratorCSG":
        # one head (level 0, pad 1); per level num_layer blocks on a volume padded by num_layer; the tail (pad 1) at the
        # level a step ends on
        head = [((nc, N), grown(sp, 2))] if lvl == 0 else []
        return head + [((N, N), grown(sp, 2 * n - 2 * i)) for i in range(n)] + [((N, nc), grown(sp, 2))]
    if net == "WDiscriminatorBaselines":
        # input padded by num_layer + 2, padd_size = 1 convs: every conv at the padded size
        assert int(opt.padd_size) == 1
        big = grown(sp, 2 * (n + 2))
        return [((nc, N), big), ((N, N), big), ((N, 1), big)]
    raise ValueError(net)


def baseline_step_groups(generator, discriminator, stage, opt=None, shapes=None):
    """{((Cin, Cout), shape)} of the conv launches (forward, backward-data and weight gradient alike) of ONE
    BaselineStageTrainer.step at `stage`: the generator's levels 0 ... stage (GeneratorCSG: one tail, after the last), and
    the critic at the stage's level - WDiscriminatorBaselines on the padded volume, WDiscriminator3D on the level shape
    itself (those are launch_groups()'s)."""
    if opt is None:
        opt, shapes = baseline_opt()
    out = set()
    for lvl in range(stage + 1):
        g = baseline_net_groups(generator, lvl, opt, shapes)
        out.update(g[:-1] if generator == "GeneratorCSG" and lvl < stage else g)
    if discriminator == "WDiscriminatorBaselines":
        out.update(baseline_net_groups(discriminator, stage, opt, shapes))
    else:
        N, nc = int(opt.nfc), int(opt.nc_im)
        out.update(((ci, co), tuple(shapes[stage])) for ci, co in ((nc, N), (N, N), (N, 1)))
    return out


def baseline_launch_groups():
    """[("baseline", level, (Cin, Cout), shape)]: every distinct (layer, shape) the three baselines networks launch over
    the eight levels of the baseline config, in level order; each is launched at B = 2."""
    opt, shapes = baseline_opt()
    assert shapes == level_shapes()["video8"], shapes
    seen, out = set(), []
    for lvl in range(len(shapes)):
        for net in BASELINE_NETS:
            for key in baseline_net_groups(net, lvl, opt, shapes):
                if key not in seen:
                    seen.add(key)
                    out.append(("baseline", lvl, key[0], key[1]))
    return out


BASELINE_B = 2


# Expected kernel kinds of the baselines' launches at B = 2, per padded shape, in the notation of KINDS with one digit per
# layer of LAYERS (3->64, 64->64, 64->3, 64->1); the host test checks all four layers at every shape, the GPU test launches
# the (layer, shape) pairs of baseline_launch_groups().  The 64->64 forward / backward-data conv leaves the two-axis kernel
# at all seven shapes of the finest level (W = 258 ... 270) and at four small shapes.
_B2 = "f0233 d3200 w4344 b0100"     # 64->64 two-axis
_B1 = "f0133 d3100 w4344 b0100"     # 64->64 forward and backward-data one-axis (the weight gradient stays two-axis)
BASELINE_KINDS = {
    # level 0 (4, 27, 48) + 2 ... + 14
    (6, 29, 50): _B1, (8, 31, 52): _B1, (10, 33, 54): _B2, (12, 35, 56): _B2, (14, 37, 58): _B2, (16, 39, 60): _B2,
    (18, 41, 62): _B2,
    # level 1 (4, 34, 61) + 2 ... + 14
    (6, 36, 63): _B1, (8, 38, 65): _B2, (10, 40, 67): _B2, (12, 42, 69): _B1, (14, 44, 71): _B2, (16, 46, 73): _B2,
    (18, 48, 75): _B2,
    # level 2 (4, 43, 78) + 2 ... + 14
    (6, 45, 80): _B2, (8, 47, 82): _B2, (10, 49, 84): _B2, (12, 51, 86): _B2, (14, 53, 88): _B2, (16, 55, 90): _B2,
    (18, 57, 92): _B2,
    # level 3 (5, 55, 99) + 2 ... + 14
    (7, 57, 101): _B2, (9, 59, 103): _B2, (11, 61, 105): _B2, (13, 63, 107): _B2, (15, 65, 109): _B2, (17, 67, 111): _B2,
    (19, 69, 113): _B2,
    # level 4 (5, 70, 125) + 2 ... + 14
    (7, 72, 127): _B2, (9, 74, 129): _B2, (11, 76, 131): _B2, (13, 78, 133): _B2, (15, 80, 135): _B2, (17, 82, 137): _B2,
    (19, 84, 139): _B2,
    # level 5 (7, 89, 159) + 2 ... + 14
    (9, 91, 161): _B2, (11, 93, 163): _B2, (13, 95, 165): _B2, (15, 97, 167): _B2, (17, 99, 169): _B2, (19, 101, 171): _B2,
    (21, 103, 173): _B2,
    # level 6 (7, 113, 202) + 2 ... + 14
    (9, 115, 204): _B2, (11, 117, 206): _B2, (13, 119, 208): _B2, (15, 121, 210): _B2, (17, 123, 212): _B2,
    (19, 125, 214): _B2, (21, 127, 216): _B2,
    # level 7 (13, 144, 256) + 2 ... + 14
    (15, 146, 258): _B1, (17, 148, 260): _B1, (19, 150, 262): _B1, (21, 152, 264): _B1, (23, 154, 266): _B1,
    (25, 156, 268): _B1, (27, 158, 270): _B1,
}


def baseline_expected_kinds(layer, sp):
    """(forward, backward-data, weight-gradient kind, fuses_bias) of BASELINE_KINDS for one B = 2 launch."""
    s = {p[0]: p[1:] for p in BASELINE_KINDS[tuple(sp)].split()}
    j = LAYERS.index(tuple(layer))
    return int(s["f"][j]), int(s["d"][j]), int(s["w"][j]), int(s["b"][j])
