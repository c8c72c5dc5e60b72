"""Float64 references of the non-conv kernels of the train step - BatchNorm (+ LeakyReLU) forward, backward and second-order
backward, the align_corners resize and its adjoint, the gradient penalty and the scalar losses - each with a per-element
error scale A, and the list of their launches in the benchmark's pyramids (tests/test_ew_launch_host.py,
tests/test_ew_launches.py).  The checker is conv_ref.check: |got_i - ref_i| <= tau * A_i per element.

Error scales.  As in conv_ref, A is the sum of the magnitudes of the terms the fp32 computation combines for that element, so
the bound holds for any summation order; every A below also carries the propagated error of the per-channel statistics
the element is built from.  u = 2^-24 is the fp32 unit roundoff.  All functions run on CPU and GPU tensors alike (torch's
own float64 ops: not libhpvg's kernels); results stay on the device of the inputs.

BatchNorm forward (per group of Bg samples, N = Bg * S elements per channel; the kernel sums fp32 runs of 32 elements
and combines them in double, then forms var = E[r^2] - mean^2 in double):
  mean = E[r], var = E[(r - mean)^2] (biased), invstd = 1/sqrt(var + eps), scale = gamma*invstd, shift = beta - mean*scale,
  h = lrelu?(gamma*(r - mean)*invstd + beta); running: rm <- (1-m) rm + m mean, rv <- (1-m) rv + m var*N/(N-1), applied
  once per group, in order.
  A(mean) = E|r|: the sums' terms.  A(var) = E[r^2]: var is a difference of E[r^2] and mean^2, so its error scales with
  E[r^2], not with var.  A(invstd) = invstd * E[r^2]/(var + eps): d invstd / invstd = -d var / (2 (var + eps)).
  A(scale) = |gamma| A(invstd).  A(shift) = |beta| + |mean| A(scale) + |scale| A(mean).
  A(rm) = (1-m)|rm| + m A(mean), A(rv) = (1-m)|rv| + m E[r^2] N/(N-1) (recursively over the groups).
  A(h_i) = |gamma| invstd (|r_i| + |mean| + A(mean)) + |beta| + |gamma| |r_i - mean| A(invstd): the terms x*scale + shift
  cancels (|scale r_i| + |shift| <= |gamma| invstd (|r_i| + |mean|) + |beta|), plus the statistics' propagated error.
  LeakyReLU is 1-Lipschitz, so the same A bounds lrelu(h).
BatchNorm backward (stats = the forward's fp32 mean, invstd, scale, shift, as the kernel reads them; z = scale*r + shift):
  dz = dh * lrelu'(z), xhat = (r - mean)*invstd, Sd = sum dz, Sdx = sum dz*xhat (per channel and group),
  dr = scale*(dz - Sd/N - xhat*Sdx/N), dbeta = sum_groups Sd, dgamma = sum_groups Sdx.
  With xa = (|r| + |mean|)*invstd (the terms of xhat) and |dz|' = |dz| + 0.8|dh| where the sign of z is within fp32
  rounding of 0 (|z| <= 4u (|scale r| + |shift|): the kernel may take either slope there):
  A(Sd) = sum |dz|', A(Sdx) = sum |dz|' xa, A(dr_i) = |scale| (|dz_i|' + A(Sd)/N + 2 xa_i A(Sdx)/N).
  The direct-slot form (accumulate into a preset .grad) adds the preset value and its magnitude.
Second-order BatchNorm (groups = 1; G = dL/d(dr); SG = sum G, SGx = sum G*xhat, SdG = sum dz*G): the closed form above
  bn_lrelu_bwd2_reduce_kernel in csrc/elementwise.hip; every A is the same expression over magnitudes (sums of |terms|).
Resize (align_corners): y = sum_taps w*x with the weights of the float64 source coordinate o*(in-1)/(out-1).  The
  kernel forms the coordinate in fp32: scale = fl((in-1)/(out-1)), src = fl(scale*o), so |src32 - src| <= 2u (in-1)
  (1 + u), its weights w1 = src32 - floor(src32) (exact) and w0 = 1 - w1 (one rounding) are off by at most
  delta = 2u (in-1) + u, and where src is within delta of an integer k the fp32 coordinate may fall on the other side of
  k, moving the taps to (k-1, k) with a weight <= delta on k-1.  So per axis a the coordinate costs at most
  delta_a * R_a(|x|), R_a = the resize with axis a's weights replaced by 1 on its taps (and on k-1, k, k+1 near an
  integer k).  The fp32 products and sums cost a few u of resize(|x|).  Hence
    A = resize(|x|) + sum_a (delta_a / TAU) * R_a(|x|),
  i.e. TAU * A = TAU * resize(|x|) + the coordinate bound.  At the finest transition (in = 204) delta / TAU = 2.4.  The
  backward is the adjoint (all matrices transposed) on |dy|; yn = y + amp*noise adds |amp*noise|.
Gradient penalty (n = B*S voxels, nrm = ||g[b,:,s]||_2): P = lam/n sum (nrm - 1)^2, A(P) = lam/n sum (nrm + 1)^2 (the
  fp32 nrm - 1 carries u (nrm + 1)).  dg = gout*lam*2/n * (nrm - 1)/nrm * g (0 where nrm = 0), A = |coef| (1 + 1/nrm)|g|.
Losses (sums of fp32 terms combined in double): MSE = mean (a - b)^2, A = mean (a - b)^2; da = 2 gout/n (a - b),
  A = |da|.  KL = mean -0.5 (1 + lv - mu^2 - e^lv), A = mean 0.5 (1 + |lv| + mu^2 + e^lv); dmu = gout mu/n,
  dlv = -0.5 gout (1 - e^lv)/n, A = |gout|/n (|mu|, 0.5 (1 + e^lv)).  sign/n * sum x: A = sum |x|/n.  sqsum: A = value.

Tolerances.  TAU (conv_ref.TAU = 1e-5) for every tensor and loss: ~100x the few-u error of fp32 arithmetic over A, and
far below what a wrong statistic, a dropped partial, a wrong mask or a missing resize contribution produces (the host test
shows each).  TAU_STAT = 1e-6 for the per-channel statistics and running buffers: each is a handful of fp32 roundings
(<= 4u = 2.4e-7 of A) of double-combined sums; the running variance updated with the biased variance is off by m var/N,
2e-5 of A at the first level at B = 1, which TAU passes and TAU_STAT does not."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import conv_ref  # noqa: E402

TAU = conv_ref.TAU
TAU_STAT = 1e-6
U = 2.0 ** -24
SLOPE = 0.2
BN_MOMENTUM = 0.1
BN_EPS = 1e-5
# BatchNorm channels of every generator / critic body layer (modules/_nets.py ConvBlock: nfc = 64)
BN_C = 64
# (B, groups) of the BatchNorm launches: one generator / critic pass, the merged rec + rand generator pass, a batch-split rank
BN_BATCHES = ((2, 1), (4, 2), (1, 1))
# channels the generator resizes from level to level (its 3-channel images, modules/_nets.py forward / forward_pair)
RESIZE_C = 3
# the baselines critic (WDiscriminatorBaselines) pads its input by num_layer + 2 = 7 on every side of every axis
PAD_BASELINES = 7


def _flat(t, groups):
    """[B, C, ...] -> [groups, B/groups, C, S] float64."""
    B, C = t.shape[0], t.shape[1]
    return t.detach().double().reshape(groups, B // groups, C, -1)


def _cs(v):
    """[G, C] per-channel values -> broadcastable over [G, Bg, C, S]."""
    return v[:, None, :, None]


# ------------------------------------------------------------------------------------------------ BatchNorm
def bn_fwd64(r, gamma, beta, running_mean, running_var, groups=1, lrelu=True, momentum=BN_MOMENTUM, eps=BN_EPS):
    """Train-mode BatchNorm (+ LeakyReLU) per group in float64 -> dict of (value, A): h [r's shape]; mean, invstd, scale,
    shift [groups, C]; rm, rv [C] (after the groups' updates, in order)."""
    x = _flat(r, groups)
    G, Bg, C, S = x.shape
    N = Bg * S
    g64 = gamma.detach().double().view(1, C)
    b64 = beta.detach().double().view(1, C)
    mean = x.mean(dim=(1, 3))
    d = x - _cs(mean)
    var = (d * d).mean(dim=(1, 3))
    ex2 = (x * x).mean(dim=(1, 3))
    meanA = x.abs().mean(dim=(1, 3))
    invstd = 1.0 / torch.sqrt(var + eps)
    invstdA = invstd * ex2 / (var + eps)
    scale = g64 * invstd
    shift = b64 - mean * scale
    scaleA = g64.abs() * invstdA
    shiftA = b64.abs() + mean.abs() * scaleA + scale.abs() * meanA
    z = d * _cs(scale.expand(G, C)) + _cs(b64.expand(G, C))
    h = conv_ref.lrelu(z, SLOPE) if lrelu else z
    del z
    hA = d.abs() * _cs((g64.abs() * invstdA)) + (x.abs() + _cs(mean.abs() + meanA)) * _cs(g64.abs() * invstd) + _cs(b64.abs().expand(G, C))
    del d
    m = float(momentum)
    rm, rv = running_mean.detach().double().clone(), running_var.detach().double().clone()
    rmA, rvA = rm.abs(), rv.abs()
    f = N / (N - 1) if N > 1 else 1.0
    for k in range(G):
        rm, rmA = (1 - m) * rm + m * mean[k], (1 - m) * rmA + m * meanA[k]
        rv, rvA = (1 - m) * rv + m * var[k] * f, (1 - m) * rvA + m * ex2[k] * f
    shape = tuple(r.shape)
    return {"h": (h.reshape(shape), hA.reshape(shape)), "mean": (mean, meanA), "invstd": (invstd, invstdA),
            "scale": (scale, scaleA), "shift": (shift, shiftA), "rm": (rm, rmA), "rv": (rv, rvA)}


def _bwd_common(dh, r, stats, groups, lrelu):
    """dz, |dz|', xhat, xa, per-group stats [G, C] (float64 of the fp32 values the kernel reads)."""
    x = _flat(r, groups)
    dhv = _flat(dh, groups)
    st = stats.detach().double().reshape(groups, 4, -1)
    mean, invstd, sc, sf = st[:, 0], st[:, 1], st[:, 2], st[:, 3]
    if lrelu:
        z = x * _cs(sc) + _cs(sf)
        m = torch.where(z > 0, torch.ones_like(z), torch.full_like(z, SLOPE))   # (python scalars would make it fp32)
        amb = z.abs() <= 4 * U * ((x * _cs(sc)).abs() + _cs(sf.abs()))
        del z
        dz = dhv * m
        dza = dz.abs() + (1 - SLOPE) * dhv.abs() * amb
        del amb
    else:
        m = None
        dz = dhv
        dza = dhv.abs()
    xh = (x - _cs(mean)) * _cs(invstd)
    xa = (x.abs() + _cs(mean.abs())) * _cs(invstd)
    return dhv, dz, dza, xh, xa, mean, invstd, sc, m


def bn_bwd64(dh, r, stats, groups=1, lrelu=True, base_gamma=None, base_beta=None):
    """Backward of BNAct given the forward's statistics ([groups, 4, C] fp32: mean, invstd, scale, shift) in float64 ->
    {"dr", "dgamma", "dbeta"} of (value, A); base_*: the preset .grad of the direct-slot form (added, with its magnitude)."""
    dhv, dz, dza, xh, xa, mean, invstd, sc, _ = _bwd_common(dh, r, stats, groups, lrelu)
    N = xh.shape[1] * xh.shape[3]
    Sd = dz.sum(dim=(1, 3))
    Sdx = (dz * xh).sum(dim=(1, 3))
    aSd = dza.sum(dim=(1, 3))
    aSdx = (dza * xa).sum(dim=(1, 3))
    dr = _cs(sc) * (dz - _cs(Sd / N) - xh * _cs(Sdx / N))
    drA = _cs(sc.abs()) * (dza + _cs(aSd / N) + 2 * xa * _cs(aSdx / N))
    db, dbA, dg, dgA = Sd.sum(0), aSd.sum(0), Sdx.sum(0), aSdx.sum(0)
    if base_beta is not None:
        b0 = base_beta.detach().double()
        db, dbA = b0 + db, b0.abs() + dbA
    if base_gamma is not None:
        g0 = base_gamma.detach().double()
        dg, dgA = g0 + dg, g0.abs() + dgA
    shape = tuple(r.shape)
    return {"dr": (dr.reshape(shape), drA.reshape(shape)), "dgamma": (dg, dgA), "dbeta": (db, dbA)}


def bn_bwd2_64(dh, G, r, stats, lrelu=True):
    """Second-order BatchNorm (groups = 1): gradients of <dr, G> w.r.t. dh, r and gamma (the closed form above
    bn_lrelu_bwd2_reduce_kernel) -> {"g_dh", "g_r", "g_gamma"} of (value, A)."""
    dhv, dz, dza, xh, xa, mean, invstd, sc, m = _bwd_common(dh, r, stats, 1, lrelu)
    Gv = _flat(G, 1)
    N = xh.shape[1] * xh.shape[3]
    Ga = Gv.abs()

    def s(t):
        return t.sum(dim=(1, 3))

    Sd, Sdx, SG, SGx, SdG = s(dz), s(dz * xh), s(Gv), s(Gv * xh), s(dz * Gv)
    aSd, aSdx, aSG, aSGx, aSdG = s(dza), s(dza * xa), s(Ga), s(Ga * xa), s(dza * Ga)
    mm = m if m is not None else 1.0
    ma = (m + (1 - SLOPE) * (dza > dz.abs())) if m is not None else 1.0   # either slope where the sign of z is uncertain
    g_dh = mm * _cs(sc) * (Gv - _cs(SG / N) - xh * _cs(SGx / N))
    g_dhA = ma * _cs(sc.abs()) * (Ga + _cs(aSG / N) + 2 * xa * _cs(aSGx / N))
    k = sc * invstd
    g_r = _cs(k) * (xh * _cs((SG * Sd / N - SdG + 3 * Sdx * SGx / N) / N) + _cs(SGx / N) * (_cs(Sd / N) - dz)
                    + _cs(Sdx / N) * (_cs(SG / N) - Gv))
    g_rA = _cs(k.abs()) * (xa * _cs((aSG * aSd / N + aSdG + 3 * aSdx * aSGx / N) / N) + _cs(aSGx / N) * (_cs(aSd / N) + dza)
                           + _cs(aSdx / N) * (_cs(aSG / N) + Ga))
    g_gamma = (invstd * (SdG - Sd * SG / N - Sdx * SGx / N))[0]
    g_gammaA = (invstd * (aSdG + aSd * aSG / N + aSdx * aSGx / N))[0]
    shape = tuple(r.shape)
    return {"g_dh": (g_dh.reshape(shape), g_dhA.reshape(shape)), "g_r": (g_r.reshape(shape), g_rA.reshape(shape)),
            "g_gamma": (g_gamma, g_gammaA)}


# ------------------------------------------------------------------------------------------------ resize (align_corners)
def axis_weights(n_in, n_out, device="cpu"):
    """(M, band, delta) of one axis: M [n_out, n_in] the float64 interpolation weights of src = o (n_in - 1)/(n_out - 1);
    band = 1 on each output's taps (and on k-1, k, k+1 where src is within delta of an integer k); delta = the fp32
    coordinate's weight error bound 2u (n_in - 1) + u."""
    o = torch.arange(n_out, dtype=torch.float64)
    src = o * (n_in - 1) / (n_out - 1) if n_out > 1 else torch.zeros(1, dtype=torch.float64)
    i0 = src.floor().long().clamp(max=n_in - 1)
    i1 = (i0 + 1).clamp(max=n_in - 1)
    w1 = src - i0.double()
    M = torch.zeros(n_out, n_in, dtype=torch.float64)
    rows = torch.arange(n_out)
    M.index_put_((rows, i0), 1 - w1, accumulate=True)
    M.index_put_((rows, i1), w1, accumulate=True)
    delta = 2 * U * (n_in - 1) * (1 + U) + U
    band = torch.zeros(n_out, n_in, dtype=torch.float64)
    band[rows, i0] = 1
    band[rows, i1] = 1
    k = src.round()
    near = (src - k).abs() <= delta
    for dk in (-1, 0, 1):
        j = (k.long() + dk).clamp(0, n_in - 1)
        band[rows[near], j[near]] = 1
    return M.to(device), band.to(device), delta


def _along(t, M, dim):
    """t with axis `dim` (length M.shape[1]) mapped through M: [.., n_in, ..] -> [.., n_out, ..]."""
    return torch.movedim(torch.movedim(t, dim, -1) @ M.t(), -1, dim)


def _apply(t, mats):
    nd = len(mats)
    for a, M in enumerate(mats):
        t = _along(t, M, t.dim() - nd + a)
    return t


def _resize_pair(t, in_sp, out_sp, adjoint):
    axes = [axis_weights(i, o, t.device) for i, o in zip(in_sp, out_sp)]
    mats = [M.t() if adjoint else M for M, _, _ in axes]
    bands = [b.t() if adjoint else b for _, b, _ in axes]
    t64 = t.detach().double()
    ref = _apply(t64, mats)
    ta = t64.abs()
    A = _apply(ta, mats)
    for a, (_, _, delta) in enumerate(axes):
        A += (delta / TAU) * _apply(ta, [bands[j] if j == a else mats[j] for j in range(len(mats))])
    return ref, A


def resize64(x, size, noise=None, amp=0.0):
    """align_corners resize of x [B, C, *in] to `size` in float64 -> (y, A), or with noise (y, A, yn, ynA)."""
    y, A = _resize_pair(x, tuple(x.shape[2:]), tuple(size), False)
    if noise is None:
        return y, A
    nz = float(amp) * noise.detach().double()
    return y, A, y + nz, A + nz.abs()


def resize_bwd64(dy, in_size, dy2=None):
    """Adjoint of the resize: dx = resize^T(dy (+ dy2)) -> (dx, A) on |dy| (+ |dy2|: the kernel adds the two in fp32)."""
    g = dy.detach().double()
    if dy2 is None:
        return _resize_pair(g, tuple(in_size), tuple(dy.shape[2:]), True)
    ref, _ = _resize_pair(g + dy2.detach().double(), tuple(in_size), tuple(dy.shape[2:]), True)
    _, A = _resize_pair(g.abs() + dy2.detach().double().abs(), tuple(in_size), tuple(dy.shape[2:]), True)
    return ref, A


# ------------------------------------------------------------------------------------------------ gradient penalty, losses
def gp64(g, lam):
    """lam * mean_{b,voxel} (||g[b,:,voxel]||_2 - 1)^2 -> (P, A) as 0-d float64 tensors."""
    g64 = g.detach().double()
    nrm = g64.pow(2).sum(dim=1).sqrt()
    n = nrm.numel()
    return lam * ((nrm - 1) ** 2).sum() / n, lam * ((nrm + 1) ** 2).sum() / n


def gp_bwd64(gout, g, lam):
    """d P / d g * gout -> (dg, A); 0 where the voxel's norm is 0."""
    g64 = g.detach().double()
    nrm = g64.pow(2).sum(dim=1, keepdim=True).sqrt()
    n = nrm.numel()
    k = float(gout) * lam * 2 / n
    safe = torch.where(nrm > 0, nrm, torch.ones_like(nrm))
    dg = torch.where(nrm > 0, k * (nrm - 1) / safe * g64, torch.zeros_like(g64))
    A = torch.where(nrm > 0, abs(k) * (1 + 1 / safe) * g64.abs(), torch.zeros_like(g64))
    return dg, A


def mse64(a, b):
    d = a.detach().double() - b.detach().double()
    v = (d * d).mean()
    return v, v.clone()


def mse_bwd64(gout, a, b):
    d = a.detach().double() - b.detach().double()
    da = 2 * float(gout) / d.numel() * d
    return da, da.abs()


def kl64(mu, lv):
    m, l = mu.detach().double(), lv.detach().double()
    e = l.exp()
    return (-0.5 * (1 + l - m * m - e)).mean(), (0.5 * (1 + l.abs() + m * m + e)).mean()


def kl_bwd64(gout, mu, lv):
    m, l = mu.detach().double(), lv.detach().double()
    k = float(gout) / m.numel()
    dmu = k * m
    dlv = -0.5 * k * (1 - l.exp())
    return (dmu, dmu.abs()), (dlv, 0.5 * abs(k) * (1 + l.exp()))


def mean_scaled64(x, sign):
    x64 = x.detach().double()
    return sign * x64.sum() / x64.numel(), x64.abs().sum() / x64.numel()


def sqsum64(x):
    v = x.detach().double().pow(2).sum()
    return v, v.clone()


# ------------------------------------------------------------------------------------------------ the pyramids' launches
def spatial(sp):
    S = 1
    for v in sp:
        S *= int(v)
    return S


def bn_launches():
    """[(config, level, shape, B, groups)]: BNAct (C = BN_C) at every distinct level shape (conv_ref.level_shapes; video8's
    finest level is video's) for every (B, groups) of BN_BATCHES."""
    seen, out = set(), []
    for cfg, shapes in conv_ref.level_shapes().items():
        for lvl, sp in enumerate(shapes):
            if sp in seen:
                continue
            seen.add(sp)
            for B, groups in BN_BATCHES:
                out.append((cfg, lvl, sp, B, groups))
    return out


def bn_plan_of(lib, B, S, groups, C=BN_C):
    """(fused, nsplit, V) the library plans for a BatchNorm launch (hpvg_bn_plan)."""
    import ctypes
    out = (ctypes.c_int * 3)()
    assert lib.hpvg_bn_plan(B, C, S, groups, out) == 0
    return tuple(int(v) for v in out)


def padded_shapes(cfg="video8", pad=PAD_BASELINES):
    """Level shapes of `cfg` with every axis grown by 2 pad: the volumes the baselines critic's BatchNorms see."""
    return [tuple(v + 2 * pad for v in sp) for sp in conv_ref.level_shapes()[cfg]]


def resize_launches():
    """[(config, level, in shape, out shape)]: the generator's level-to-level resizes of every pyramid (level i -> i + 1)."""
    out = []
    for cfg, shapes in conv_ref.level_shapes().items():
        for lvl in range(len(shapes) - 1):
            out.append((cfg, lvl, shapes[lvl], shapes[lvl + 1]))
    return out


# (fused, nsplit, V) of every BatchNorm launch (C = 64), per level shape for the (B, groups) of BN_BATCHES: (2, 1), (4, 2),
# (1, 1).  fused = 1: the finalize folded into the apply kernel, 0: three launches per group; nsplit = partial blocks per
# channel and group; V = vector width of the reduction kernels (S = T*H*W: 4 when S % 4 == 0, 2 when even, else 1).  A
# change of the size rules (bn_nsplit, HPVG_BN_FUSE_MAX, hpvg_vec_width) must change this table on purpose: it decides which
# path and which reduction kernel each launch of tests/test_ew_launches.py exercises.
BN_PLANS = {
    # video (configs[2])
    (4, 18, 33): ((1, 3, 4), (1, 3, 4), (1, 2, 4)), (4, 23, 41): ((1, 4, 4), (1, 4, 4), (1, 2, 4)),
    (4, 28, 51): ((1, 6, 4), (1, 6, 4), (1, 3, 4)), (5, 36, 65): ((1, 12, 4), (1, 12, 4), (1, 6, 4)),
    (5, 45, 81): ((1, 16, 1), (1, 16, 1), (1, 9, 1)), (5, 57, 102): ((1, 16, 2), (1, 16, 2), (1, 15, 2)),
    (7, 72, 129): ((1, 16, 4), (1, 16, 4), (1, 16, 4)), (7, 91, 162): ((1, 16, 2), (1, 16, 2), (1, 16, 2)),
    (7, 114, 204): ((1, 16, 4), (0, 16, 4), (1, 16, 4)), (13, 144, 256): ((0, 16, 4), (0, 16, 4), (1, 16, 4)),
    # video8 (configs[3]); its finest level is video's
    (4, 27, 48): ((1, 6, 4), (1, 6, 4), (1, 3, 4)), (4, 34, 61): ((1, 9, 4), (1, 9, 4), (1, 5, 4)),
    (4, 43, 78): ((1, 14, 4), (1, 14, 4), (1, 7, 4)), (5, 55, 99): ((1, 16, 1), (1, 16, 1), (1, 14, 1)),
    (5, 70, 125): ((1, 16, 2), (1, 16, 2), (1, 16, 2)), (7, 89, 159): ((1, 16, 1), (1, 16, 1), (1, 16, 1)),
    (7, 113, 202): ((1, 16, 2), (0, 16, 2), (1, 16, 2)),
    # image (configs[1], 2-D: S = H*W)
    (24, 33): ((1, 1, 4), (1, 1, 4), (1, 1, 4)), (30, 41): ((1, 2, 2), (1, 2, 2), (1, 1, 2)),
    (38, 51): ((1, 2, 2), (1, 2, 2), (1, 1, 2)), (48, 65): ((1, 4, 4), (1, 4, 4), (1, 2, 4)),
    (60, 81): ((1, 5, 4), (1, 5, 4), (1, 3, 4)), (76, 102): ((1, 8, 4), (1, 8, 4), (1, 4, 4)),
    (96, 129): ((1, 13, 4), (1, 13, 4), (1, 7, 4)), (121, 162): ((1, 16, 2), (1, 16, 2), (1, 10, 2)),
    (153, 204): ((1, 16, 4), (1, 16, 4), (1, 16, 4)), (192, 256): ((1, 16, 4), (1, 16, 4), (1, 16, 4)),
}
# the second-order BatchNorm's launches: the baselines critic's padded video8 volumes at B = 2 (groups = 1)
BN2_PLANS = {
    (18, 41, 62): (1, 16, 4), (18, 48, 75): (1, 16, 4), (18, 57, 92): (1, 16, 4), (19, 69, 113): (1, 16, 1),
    (19, 84, 139): (1, 16, 4), (21, 103, 173): (0, 16, 1), (21, 127, 216): (0, 16, 4), (27, 158, 270): (0, 16, 4),
}


def expected_plan(sp, B, groups):
    return BN_PLANS[tuple(sp)][BN_BATCHES.index((B, groups))]


# ------------------------------------------------------------------------------------------------ the baselines' launches
def baseline_bn_shapes():
    """[(level, shape)]: what the baselines' BatchNorms see at B = 2 beyond the level shapes themselves - the cropped conv
    outputs level + 12 ... + 2 (GeneratorSG's head and blocks, GeneratorCSG's blocks) and level + 14 (WDiscriminatorBaselines:
    padding-1 convs on the padded input).  level + 0 (the last block, GeneratorCSG's head) is in bn_launches()."""
    opt, shapes = conv_ref.baseline_opt()
    full = 2 * (int(opt.num_layer) + 2)
    return [(lvl, conv_ref.grown(sp, k)) for lvl, sp in enumerate(shapes) for k in range(2, full + 1, 2)]


def baseline_resize_launches():
    """[(level, C, in shape, out shape, in-kernel noise)] of the baselines generators' level i -> i + 1 resizes at B = 2:
    GeneratorSG resizes its 3-channel image to the level and, with noise made in the kernel, straight to the padded size
    level + 2 (num_layer + 2); GeneratorCSG its nfc-channel features to the level and, with noise, to level + 2 num_layer.
    (The plain 3-channel level -> level resize is resize_launches()'s.)"""
    opt, shapes = conv_ref.baseline_opt()
    n, N, nc = int(opt.num_layer), int(opt.nfc), int(opt.nc_im)
    out = []
    for lvl in range(len(shapes) - 1):
        a, b = shapes[lvl], shapes[lvl + 1]
        out.append((lvl, nc, a, conv_ref.grown(b, 2 * (n + 2)), True))
        out.append((lvl, N, a, b, False))
        out.append((lvl, N, a, conv_ref.grown(b, 2 * n), True))
    return out


def all_level_shapes():
    """[(config, level, shape)] of all four configs (video, video8, image, baseline = video8's shapes), distinct shapes once."""
    seen, out = set(), []
    for cfg, shapes in conv_ref.level_shapes().items():
        for lvl, sp in enumerate(shapes):
            if sp not in seen:
                seen.add(sp)
                out.append((cfg, lvl, sp))
    return out


# (fused, nsplit, V) of the baselines' first-order BatchNorm launches (B = 2, C = 64, groups = 1) at the shapes of
# baseline_bn_shapes(), in the notation of BN_PLANS.  (0, 16, 1) - three launches per group with scalar loads - is reached
# by no launch of BN_PLANS.
BASELINE_BN_PLANS = {
    # level 0 (4, 27, 48) + 2 ... + 14
    (6, 29, 50): (1, 9, 4), (8, 31, 52): (1, 13, 4), (10, 33, 54): (1, 16, 4), (12, 35, 56): (1, 16, 4),
    (14, 37, 58): (1, 16, 4), (16, 39, 60): (1, 16, 4), (18, 41, 62): (1, 16, 4),
    # level 1 (4, 34, 61) + 2 ... + 14
    (6, 36, 63): (1, 14, 4), (8, 38, 65): (1, 16, 4), (10, 40, 67): (1, 16, 4), (12, 42, 69): (1, 16, 4),
    (14, 44, 71): (1, 16, 4), (16, 46, 73): (1, 16, 4), (18, 48, 75): (1, 16, 4),
    # level 2 (4, 43, 78) + 2 ... + 14
    (6, 45, 80): (1, 16, 4), (8, 47, 82): (1, 16, 4), (10, 49, 84): (1, 16, 4), (12, 51, 86): (1, 16, 4),
    (14, 53, 88): (1, 16, 4), (16, 55, 90): (1, 16, 4), (18, 57, 92): (1, 16, 4),
    # level 3 (5, 55, 99) + 2 ... + 14
    (7, 57, 101): (1, 16, 1), (9, 59, 103): (1, 16, 1), (11, 61, 105): (1, 16, 1), (13, 63, 107): (1, 16, 1),
    (15, 65, 109): (1, 16, 1), (17, 67, 111): (1, 16, 1), (19, 69, 113): (1, 16, 1),
    # level 4 (5, 70, 125) + 2 ... + 14
    (7, 72, 127): (1, 16, 4), (9, 74, 129): (1, 16, 2), (11, 76, 131): (1, 16, 4), (13, 78, 133): (1, 16, 2),
    (15, 80, 135): (1, 16, 4), (17, 82, 137): (1, 16, 2), (19, 84, 139): (1, 16, 4),
    # level 5 (7, 89, 159) + 2 ... + 14
    (9, 91, 161): (1, 16, 1), (11, 93, 163): (1, 16, 1), (13, 95, 165): (1, 16, 1), (15, 97, 167): (1, 16, 1),
    (17, 99, 169): (0, 16, 1), (19, 101, 171): (0, 16, 1), (21, 103, 173): (0, 16, 1),
    # level 6 (7, 113, 202) + 2 ... + 14
    (9, 115, 204): (1, 16, 4), (11, 117, 206): (0, 16, 2), (13, 119, 208): (0, 16, 4), (15, 121, 210): (0, 16, 2),
    (17, 123, 212): (0, 16, 4), (19, 125, 214): (0, 16, 2), (21, 127, 216): (0, 16, 4),
    # level 7 (13, 144, 256) + 2 ... + 14
    (15, 146, 258): (0, 16, 4), (17, 148, 260): (0, 16, 4), (19, 150, 262): (0, 16, 4), (21, 152, 264): (0, 16, 4),
    (23, 154, 266): (0, 16, 4), (25, 156, 268): (0, 16, 4), (27, 158, 270): (0, 16, 4),
}
