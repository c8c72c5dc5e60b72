"""Float64 references of the parameter-side kernels of a train step - the spectral-norm power iteration and its backward, the
gradient clip and the Adam step (csrc/elementwise.hip) - each with a per-element error scale A, and their launches as plain
data (tests/test_param_launch_host.py, tests/test_param_launches.py).  The checker is conv_ref.check:
|got_i - ref_i| <= tau * A_i per element, tau = conv_ref.TAU.

Error scales.  As in conv_ref and ew_ref, A is the sum of the magnitudes of the terms the fp32 computation combines for that
element, so the bound holds for any summation order.  u = 2^-24 is the fp32 unit roundoff.  All functions run on CPU and GPU
tensors alike (torch's own float64 ops); results stay on the device of the inputs.

Spectral norm, forward (W = weight_orig as [Co, K], one power iteration, torch.nn.utils.spectral_norm semantics).  Every
stage is judged against float64 computed from the kernel's own fp32 output of the stage before, so no error travels through
the chain and no A has to carry a propagated term:
  v  = t / max(||t||, eps), t = W^T u_in          from (W, u_in):
       A(v_k) = sum_o |w_ok| |u_o| / den + |v_k|: the terms of the dot over den, plus the rounding of the norm and of the
       division (a few u of |v_k|; the norm is summed in double from the fp32 t).
  u' = s / max(||s||, eps), s = W v               from (W, got v):  A(u'_o) = sum_k |w_ok| |v_k| / den + |u'_o|.
  sigma = u'^T W v                                from (W, got u', got v):  A = sum_ok |u'_o| |w_ok| |v_k|.
  1/sigma                                         A = A(sigma) / sigma^2 + |1/sigma|  (d(1/s) = -ds / s^2, one rounding).
  w_eff = W / got sigma                           one correctly rounded fp32 divide: A = |w_eff|, and also judged at ONE
       rounding (tau = U1 = u (1 + 2^-20)): |fl(x) - x| <= u |x| for round-to-nearest.
  With do_iter = 0 (eval mode) u and v stay as they are, bit for bit, and sigma = u^T W v is judged as above from (W, u, v).
  The (u, v) copy for the backward equals the u / v buffers bit for bit.
Spectral norm, backward (sigma, u, v = the fp32 values the forward saved; D = sum_ok dW_ok W_ok, summed in double):
  dW_orig_ok (+)= dW_ok / sigma - (D / sigma^2) u_o v_k
  A = |dW_ok| / sigma + (sum |dW| |W_orig| / sigma^2) |u_o v_k|  (+ |preset| in the accumulate form).
Clip (sq = the fp32 sum of squares the kernel reads, max_norm = the fp32 value the ABI receives):
  total = sqrt(sq), coef = min(1, max_norm / (total + 1e-6)), g *= coef.  A = |value| for each (a handful of roundings; the
  fp32 1e-6f differs from 1e-6 by 2.3e-14, far below u * total for every total the tests use, and coef = 1 exactly when
  total = 0).  When coef == 1, g comes back bit for bit.
Adam (one step from (p, g, m, v, t); lr, beta1, beta2, eps are the fp32 values the ABI receives, widened to float64:
  fl32(0.999) = 0.999000012874603 is the kernel's beta2, not 0.999):
  m' = beta1 m + (1 - beta1) g              A = |beta1 m| + |(1 - beta1) g|      (1 - beta is exact in fp32: Sterbenz)
  v' = beta2 v + (1 - beta2) g^2            A = |beta2 v| + (1 - beta2) g^2
  upd = (lr / bc1) m' / (sqrt(v') / sqrt(bc2) + eps), bc_i = 1 - beta_i^t, judged as p - p' against float64 from the
  kernel's own fp32 m', v' (m' may cancel, so its error does not belong in the update's scale).  Three kinds of error meet:
    - the update's own arithmetic (a divide, a square root, two more divides, a product): a few u of |upd|;
    - the fp32 bias corrections.  fl(beta^t) is off by u beta^t (a correctly rounded power), 1 - fl(beta^t) adds u (1 -
      beta^t), so bc loses c(beta, t) = u (beta^t + 1 - beta^t) / (1 - beta^t) <= u (1 + beta^t) / (1 - beta^t) relative:
      the subtraction cancels, and at t = 1, beta2 = 0.999 this is 2000 u = 1.2e-4, i.e. above TAU.  upd is proportional
      to 1/bc1 and, through the denominator, at most to sqrt(bc2): relative c(beta1, t) + c(beta2, t) / 2;
    - storing p' = fl(p - upd): at most u (|p| + |upd|), whatever the size of the update.
  So TAU * A(upd) = TAU |upd| + (c(beta1, t) + c(beta2, t) / 2) |upd| + u (|p| + |upd|).  The last term is a rounding
  bound, not a tolerance: it is 6e-8 |p|, where |p| itself would admit 1e-5 |p| - 2 % of an update of lr = 5e-4.  Where
  p = 0 (the tests keep such elements) it vanishes and the update is judged alone.
  Measured on an MI355X (profiles/param_launches.txt): the kernel's 1 - powf(beta, t) stays inside this bound at every t
  tested (1, 2, 3, 10, 1000, 100000); where p = 0 the worst |got - ref| / A is 1.1e-6 (t = 3), a tenth of TAU.  At t = 1
  powf(beta, 1) = beta and 1 - beta is exact.  A bias correction off by 3e-5 is rejected from t = 10 on; at t = 1, 2, 3 the
  derived conditioning of 1 - beta2^t (6e-5, 3e-5, 2e-5) is larger than that.

Tolerances.  TAU (conv_ref.TAU = 1e-5) for everything: ~100x the few-u error of fp32 arithmetic over A and far below what a
dropped row slice, a stale u, a partial dot, a shifted row index, a bias correction at t - 1, a moment without its
(1 - beta2) factor or a double-precision 1 - 0.999 produce (the host test shows each)."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import conv_ref  # noqa: E402

TAU = conv_ref.TAU
U = 2.0 ** -24
U1 = U * (1 + 2.0 ** -20)     # one correctly rounded fp32 operation: |fl(x) - x| <= u |x|
SN_EPS = 1e-12
SN_CHUNK = 4096               # elements per workgroup of the spectral-norm backward (csrc/elementwise.hip)

# ------------------------------------------------------------------------------------------------ launches as plain data
# (Co, K) of the spectral-norm layers a critic hands to ONE SpectralNormWeightBatch launch (modules/_nets.py sn_weights:
# head + num_layer = 5 body blocks at nfc = 64; K = Cin * taps; the tail is a plain conv)
SN_LAYERS_3D = ((64, 81), (64, 1728), (64, 1728), (64, 1728), (64, 1728), (64, 1728))
SN_LAYERS_2D = ((64, 27), (64, 576), (64, 576), (64, 576), (64, 576), (64, 576))
# the same batch with a one-channel last layer (a spectrally normalised tail: Co = 1, so its v is the unaligned tail
# uv + 1 of the backward's (u, v) copy, and its backward is one workgroup beside the others' 27 / 9)
SN_TAIL_3D = ((64, 81), (64, 1728), (64, 1728), (64, 1728), (64, 1728), (1, 1728))
SN_TAIL_2D = ((64, 27), (64, 576), (64, 576), (64, 576), (64, 576), (1, 576))
# floats of the ParamArena of the video config's networks (bench._video_opt; every parameter starts on a 64-float boundary):
# the generator at stage 1 (the last stage that trains encoder and decoder) and at the last stage (9), the critic; and the
# (lo, hi, lr) Adam ranges of FlatAdam over train.generator_param_groups: at stage 1 encode and decoder at lr_g * lr_scale
# and the new body block at lr_g (two learning rates), at stage 9 the last body block alone
ARENA_FLOATS = {"G1": 2014272, "G9": 6530624, "D": 560320}
ADAM_RANGES = {"G1": ((0, 669184, 1e-4), (669184, 1449728, 1e-4), (1449728, 2014272, 5e-4)), "G9": ((5966080, 6530624, 5e-4),)}


def _f32(x):
    """The fp32 value an ABI argument of type float receives, as a Python float."""
    return float(torch.tensor(float(x), dtype=torch.float32))


def _mat(w):
    return w.detach().double().reshape(w.shape[0], -1)


# ------------------------------------------------------------------------------------------------ spectral norm
def sn_normalized64(W, x, eps=SN_EPS, transpose=False):
    """y = M x / max(||M x||, eps) with M = W^T (transpose) or W, in float64 -> (y, A)."""
    M = _mat(W)
    if transpose:
        M = M.t()
    x64 = x.detach().double()
    t = M @ x64
    den = torch.clamp(t.norm(), min=float(eps))
    y = t / den
    return y, (M.abs() @ x64.abs()) / den + y.abs()


def sn_v64(W, u_in, eps=SN_EPS):
    return sn_normalized64(W, u_in, eps, transpose=True)


def sn_u64(W, v, eps=SN_EPS):
    return sn_normalized64(W, v, eps, transpose=False)


def sn_sigma64(W, u, v):
    """sigma = u^T W v and 1/sigma -> ((sigma, A), (1/sigma, A)) as 0-d float64 tensors."""
    M = _mat(W)
    u64, v64 = u.detach().double(), v.detach().double()
    sig = u64 @ (M @ v64)
    A = u64.abs() @ (M.abs() @ v64.abs())
    return (sig, A), (1.0 / sig, A / (sig * sig) + (1.0 / sig).abs())


def sn_weff64(W, sigma):
    """W / sigma (sigma: the kernel's fp32 value) -> (w_eff, A)."""
    w = W.detach().double() / sigma.detach().double().reshape(())
    return w, w.abs()


def sn_bwd64(dW, W_orig, sigma, u, v, preset=None):
    """dW_orig = dW/sigma - (sum(dW .* W_orig)/sigma^2) u v^T (+ preset) from the forward's fp32 sigma, u, v -> (value, A)."""
    d = _mat(dW)
    M = _mat(W_orig)
    s = sigma.detach().double().reshape(())
    uv = torch.outer(u.detach().double(), v.detach().double())
    dot = (d * M).sum()
    dotA = (d.abs() * M.abs()).sum()
    val = d / s - (dot / (s * s)) * uv
    A = d.abs() / s.abs() + (dotA / (s * s)) * uv.abs()
    if preset is not None:
        p = _mat(preset)
        val, A = val + p, A + p.abs()
    return val.reshape(dW.shape), A.reshape(dW.shape)


# ------------------------------------------------------------------------------------------------ clip
def clip64(sqsum, max_norm):
    """(total, coef) of clip_grad_norm_ from the fp32 sum of squares -> ((total, A), (coef, A)) as 0-d float64 tensors."""
    sq = sqsum.detach().double().reshape(())
    total = sq.sqrt()
    coef = torch.clamp(_f32(max_norm) / (total + 1e-6), max=1.0)
    return (total, total.abs()), (coef, coef.abs())


def clip_apply64(g, coef):
    r = g.detach().double() * coef
    return r, r.abs()


# ------------------------------------------------------------------------------------------------ Adam
def bias_conditioning(beta, t):
    """c(beta, t) = u (1 + beta^t) / (1 - beta^t): the relative error of the fp32 1 - beta^t (beta: the fp32 value)."""
    bt = _f32(beta) ** int(t)
    return U * (1 + bt) / (1 - bt)


def adam_moments64(g, m, v, beta1, beta2):
    """m' and v' of one Adam step -> ((m', A), (v', A)); beta1, beta2 are rounded to fp32 first, as the ABI does."""
    b1, b2 = _f32(beta1), _f32(beta2)
    g64, m64, v64 = g.detach().double(), m.detach().double(), v.detach().double()
    m1, m2 = b1 * m64, (1 - b1) * g64
    v1, v2 = b2 * v64, (1 - b2) * g64 * g64
    return (m1 + m2, m1.abs() + m2.abs()), (v1 + v2, v1.abs() + v2)


def adam_update64(p, m_new, v_new, t, lr, beta1, beta2, eps):
    """upd = p - p' of the step that left the moments (m_new, v_new) (the kernel's own fp32 values) -> (upd, A), see the
    module docstring: TAU A = TAU |upd| + (c(beta1, t) + c(beta2, t) / 2) |upd| + u (|p| + |upd|)."""
    b1, b2, lr32, eps32 = _f32(beta1), _f32(beta2), _f32(lr), _f32(eps)
    t = int(t)
    bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
    upd = (lr32 / bc1) * m_new.detach().double() / (v_new.detach().double().sqrt() / bc2 ** 0.5 + eps32)
    cond = bias_conditioning(b1, t) + 0.5 * bias_conditioning(b2, t)
    a = upd.abs()
    return upd, a * (1 + cond / TAU) + (U / TAU) * (p.detach().double().abs() + a)


def adam_step64(p, g, m, v, t, lr, beta1, beta2, eps):
    """One whole step in float64 (for the comparison with torch.optim.Adam): (p', m', v')."""
    (m1, _), (v1, _) = adam_moments64(g, m, v, beta1, beta2)
    upd, _ = adam_update64(p, m1, v1, t, lr, beta1, beta2, eps)
    return p.detach().double() - upd, m1, v1


# ------------------------------------------------------------------------------------------------ the modules' launches
def sn_layers_of(net):
    """[(Co, K)] of the SNConv layers of a critic, in the order sn_weights receives them."""
    blocks = [net.head] + list(net.body)
    return tuple((b.conv.weight_orig.shape[0], b.conv.weight_orig[0].numel()) for b in blocks)


def video_nets(stage):
    """(opt, netG, netD) of the benchmark's video config at `stage`, on CPU."""
    import copy
    import bench
    from hp_vae_gan_amd.modules import networks_3d
    torch.manual_seed(0)
    opt = bench._video_opt("cpu")
    bench._HipGeom.adjust_scales2image(opt.img_size, opt)
    opt.stop_scale_time = opt.stop_scale
    proto = networks_3d.GeneratorHPVAEGAN(opt)
    for _ in range(stage):
        proto.init_next_stage()
    opt.scale_idx = stage
    netG = copy.deepcopy(proto)
    netG.opt = opt
    return opt, netG, networks_3d.WDiscriminator3D(opt)
