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
