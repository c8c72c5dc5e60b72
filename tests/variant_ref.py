"""Float64 references of the kernels of csrc/variants.hip - the sigmoid gate, the global average pool, code x map, the relaxed
Bernoulli reparameterisation and its KL term (Encode3DVAE_nb / GeneratorVAE_nb: networks_3d.py:38-45,110-138,409-485;
losses.py:12-14) - each with a per-element error scale A by the rule of ew_ref.py (tests/test_variant_launch_host.py,
tests/test_variant_launches.py).  The checker is conv_ref.check: |got_i - ref_i| <= TAU * A_i per element, TAU = ew_ref.TAU.

Every function takes and returns tensors shaped [B, C, S] / [B, S] / [B, C] (or flat, for the two Bernoulli formulas), runs on
CPU and GPU tensors alike (torch's own float64 ops) and returns (value, A) pairs.  u = 2^-24 is the fp32 unit roundoff; A is
the sum of the magnitudes of the terms the fp32 computation combines for that element, so the bound holds for any summation
order and with or without fused multiply-adds.

Constants.  C20 = float64(float32(1e-20)) and L5 = float64(float32(log 0.5)): the values the kernels add and subtract.

Gate (gate_fwd_kernel / gate_bwd_kernel), g = sigmoid(l) = 1 / (1 + e^-l):
  bern = g.  e^-l carries the few u of expf, 1 + e one rounding, the quotient one more: a relative error of a few u.  A = g.
  out = g * f: one product of the kernel's fp32 g.  A = |g f| (the relative error of g is that of the product).
  df = dout * bern: ONE product of two fp32 values the kernel reads.  The reference takes bern as the kernel reads it (the
    forward's fp32 output), so nothing of the forward's error is in it.  A = |dout bern|.
  dlogit = (sum_c dout f + dbern_ext) * bern * (1 - bern), again with the kernel's own fp32 bern; 1 - bern is exact or one
    rounding of an fp32 value.  A = (sum_c |dout f| + |dbern_ext|) * bern * (1 - bern).
Row sum (rowsum_kernel: the pool's forward with scale = 1/S, code x map's gradient for the code with the map as weight):
  out[b, c] = scale * sum_s x[b, c, s] (w[b, s]): fp32 products summed in double, one rounding to fp32; the fp32 scale is 1/S
  within u.  A = |scale| sum_s |x w|.
Outer product (outer_kernel: code x map, and the pool's backward with scale = 1/S): out = g[b, c] * w[b, s] or g[b, c] * scale,
  one product.  A = |g w| or |g| * scale.
Column sum (colsum_kernel: code x map's gradient for the map): out[b, s] = sum_c a[b, c, s] v[b, c] in fp32.
  A = sum_c |a v|.
Reparameterisation (reparam_bern_fwd_kernel): z = log(x + C20) - log(t), t = -log(eps + C20) + C20.
  Each sum under a log is rounded once (relative error <= u; where the sum is x or eps itself to within C20 the error is C20),
  and t also carries logf's relative error of log(eps + C20): the arguments of both logs are off by at most 2u relatively, which
  moves each log by 2u ABSOLUTELY, whatever its size.  A = |log(x + C20)| + |log t| + 4.
  At the edges: x = 0 gives log C20 = -46.05, eps = 0 gives t = 46.05, eps = 1 - 2^-24 gives t = 5.96e-8 (eps + C20 rounds to
  eps exactly, and logf next to 1 is accurate relative to its small result): z is finite at all of them.
  Backward: dx = dz / (x + C20), a quotient of a once-rounded sum.  A = |dz| / (x + C20); at x = 0, 1e20 |dz|, finite in fp32.
KL (kl_bern_partial_kernel + sum_finish_kernel): mean_i [ x (log(x + C20) - L5) + (1 - x)(log(1 - x + C20) - L5) ], fp32 terms
  summed in double.  1 - x + C20 is two roundings, x + C20 one: each log moves by at most 2u absolutely.  Per element
  A_i = |x| (|log(x + C20)| + |L5| + 2) + |1 - x| (|log(1 - x + C20)| + |L5| + 2), A = mean A_i.
  Backward: dx = k (log(x + C20) + x / (x + C20) - log(1 - x + C20) - (1 - x) / (1 - x + C20)), k = gout / n in fp32.
  A = |k| (|log(x + C20)| + |log(1 - x + C20)| + x / (x + C20) + |1 - x| / (1 - x + C20) + 4).
  x = 0 and x = 1 put C20 alone under one log (-46.05) next to a factor or a quotient that is exactly 0: finite."""
import numpy as np
import torch

import conv_ref
import ew_ref

TAU = ew_ref.TAU
C20 = float(np.float32(1e-20))
L5 = float(np.float32(-0.6931471805599453))
# the inputs at which the Bernoulli formulas meet their + 1e-20 terms
X_EDGES = (0.0, 1.0, 2.0 ** -24, 1.0 - 2.0 ** -24, 1e-30)
EPS_EDGES = (0.0, 1.0 - 2.0 ** -24)


def _d(t):
    return t.detach().double()


# ------------------------------------------------------------------------------------------------ gate
def gate_fwd64(f, logit):
    """f [B, C, S], logit [B, S] -> {"out": [B, C, S], "bern": [B, S]} of (value, A)."""
    g = torch.sigmoid(_d(logit))
    out = g[:, None, :] * _d(f)
    return {"out": (out, out.abs()), "bern": (g, g.clone())}


def gate_bwd64(dout, f, bern, dbern_ext, drop_channel=None, keep_factor=True):
    """Backward of the gate from the kernel's own fp32 bern [B, S]; dout [B, C, S] or None, dbern_ext [B, S] or None ->
    {"df": [B, C, S], "dlogit": [B, S]} of (value, A).  drop_channel / keep_factor seed the host test's defects."""
    g = _d(bern)
    f64 = _d(f)
    d = _d(dout) if dout is not None else torch.zeros_like(f64)
    prod = d * f64
    if drop_channel is not None:
        keep = torch.ones(f64.shape[1], dtype=torch.float64, device=f64.device)
        keep[drop_channel] = 0
        prod = prod * keep[None, :, None]
    acc, accA = prod.sum(1), prod.abs().sum(1)
    if dbern_ext is not None:
        acc, accA = acc + _d(dbern_ext), accA + _d(dbern_ext).abs()
    fac = g * (1 - g) if keep_factor else g
    df = d * g[:, None, :]
    return {"df": (df, df.abs()), "dlogit": (acc * fac, accA * fac.abs())}


# ------------------------------------------------------------------------------------------------ pool, code x map
def rowsum64(x, w, scale):
    """out[b, c] = scale * sum_s x[b, c, s] (* w[b, s]) -> (value, A), [B, C]."""
    t = _d(x) if w is None else _d(x) * _d(w)[:, None, :]
    return scale * t.sum(2), abs(scale) * t.abs().sum(2)


def outer64(g, w, scale, S):
    """out[b, c, s] = g[b, c] * (w[b, s] or scale) -> (value, A), [B, C, S]."""
    g64 = _d(g)
    if w is None:
        out = (g64 * scale)[:, :, None].expand(g64.shape[0], g64.shape[1], S).contiguous()
    else:
        out = g64[:, :, None] * _d(w)[:, None, :]
    return out, out.abs()


def colsum64(a, v):
    """out[b, s] = sum_c a[b, c, s] v[b, c] -> (value, A), [B, S]."""
    t = _d(a) * _d(v)[:, :, None]
    return t.sum(1), t.abs().sum(1)


def pool_fwd64(x, with_scale=True):
    S = x.shape[2]
    return rowsum64(x, None, 1.0 / S if with_scale else 1.0)


def pool_bwd64(g, S):
    return outer64(g, None, 1.0 / S, S)


# ------------------------------------------------------------------------------------------------ relaxed Bernoulli
def reparam_bern_fwd64(x, eps):
    x64, e64 = _d(x), _d(eps)
    l1 = torch.log(x64 + C20)
    lt = torch.log(-torch.log(e64 + C20) + C20)
    return l1 - lt, l1.abs() + lt.abs() + 4


def reparam_bern_bwd64(dz, x):
    dx = _d(dz) / (_d(x) + C20)
    return dx, dx.abs()


def _kl_terms(x64, swapped=False):
    l1, l2 = torch.log(x64 + C20), torch.log(1 - x64 + C20)
    if swapped:                       # the host test's defect: the second term weighted by x instead of 1 - x
        val = x64 * (l1 - L5) + x64 * (l2 - L5)
    else:
        val = x64 * (l1 - L5) + (1 - x64) * (l2 - L5)
    A = x64.abs() * (l1.abs() + abs(L5) + 2) + (1 - x64).abs() * (l2.abs() + abs(L5) + 2)
    return val, A


def kl_bern_fwd64(x, swapped=False):
    """-> (value, A) as 0-d float64 tensors."""
    val, A = _kl_terms(_d(x), swapped)
    return val.mean(), A.mean()


def kl_bern_bwd64(gout, x):
    x64 = _d(x)
    k = float(gout) / x64.numel()
    l1, l2 = torch.log(x64 + C20), torch.log(1 - x64 + C20)
    q1, q2 = x64 / (x64 + C20), (1 - x64) / (1 - x64 + C20)
    return k * (l1 + q1 - l2 - q2), abs(k) * (l1.abs() + l2.abs() + q1.abs() + q2.abs() + 4)


def edge_inputs(n, gen, device="cpu"):
    """x in (0, 1) and eps in [0, 1), n >= 16 fp32 values each, with X_EDGES at the front of x and every (x edge, eps edge)
    pair covered: eps cycles through EPS_EDGES under the x edges, and the x edges repeat under a second block of eps edges."""
    x = torch.rand(n, generator=gen, device=device) * 0.98 + 0.01
    eps = torch.rand(n, generator=gen, device=device)
    k = 0
    for xe in X_EDGES:
        for ee in EPS_EDGES:
            x[k], eps[k] = xe, ee
            k += 1
    for xe in X_EDGES:                # the x edges against an ordinary eps too
        x[k] = xe
        k += 1
    assert k <= n
    return x, eps


def check(got, ref, A, what, **kw):
    """conv_ref.check at TAU."""
    return conv_ref.check(got, ref, A, what, tau=TAU, **kw)
