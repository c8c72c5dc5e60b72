"""Float64 references of the tap-generic conv family (hpvg_convk_*): tests/conv_ref.py's three references and their
absolute-value twins A, generalised from padding 1 to padding K // 2 for a cubic weight of side K (3, 5, 7), 2-D and 3-D.

|got - ref| <= TAU * A per element, with conv_ref.TAU and conv_ref.check; see conv_ref.py for why the bound scales with the
sum of the products' magnitudes.  The *_taps functions restate the same operations as a plain sum over taps of channel
matmuls on shifted views of the zero-padded input (no torch conv at all): tests/test_conv_taps_host.py pins one against the
other."""
import itertools

import torch
import torch.nn.functional as F

from conv_ref import TAU, check, err_ratio, lrelu  # noqa: F401  (re-exported for the tests of this family)


def side(w_shape):
    k = int(w_shape[2])
    assert tuple(w_shape[2:]) == (k,) * (len(w_shape) - 2) and k % 2 == 1, tuple(w_shape)
    return k


def _conv(x, w, p):
    return F.conv3d(x, w, padding=p) if x.dim() == 5 else F.conv2d(x, w, padding=p)


def _conv_input(shape, w, dy, p):
    g = torch.nn.grad.conv3d_input if dy.dim() == 5 else torch.nn.grad.conv2d_input
    return g(shape, w, dy, padding=p)


def _conv_weight(x, w_shape, dy, p):
    g = torch.nn.grad.conv3d_weight if dy.dim() == 5 else torch.nn.grad.conv2d_weight
    return g(x, w_shape, dy, padding=p)


def conv_fwd64(x, w, b=None):
    """y = conv(x, w) + b with zero padding K // 2, in float64 -> (y, A)."""
    p = side(w.shape) // 2
    x64, w64 = x.detach().double().cpu(), w.detach().double().cpu()
    y, A = _conv(x64, w64, p), _conv(x64.abs(), w64.abs(), p)
    if b is not None:
        b64 = b.detach().double().cpu().view(1, -1, *([1] * (x.dim() - 2)))
        y = y + b64
        A = A + b64.abs()
    return y, A.float()


def conv_bwd_data64(dy, w):
    """dx = conv_input(dy, w): the backward-data conv of the layer weight w, in float64 -> (dx, A)."""
    p = side(w.shape) // 2
    d64, w64 = dy.detach().double().cpu(), w.detach().double().cpu()
    shape = (dy.shape[0], w.shape[1]) + tuple(dy.shape[2:])
    return _conv_input(shape, w64, d64, p), _conv_input(shape, w64.abs(), d64.abs(), p).float()


def conv_bwd_weight64(dy, x, w_shape):
    """dw = conv_weight(x, dy) over all samples, in float64 -> (dw, A)."""
    p = side(w_shape) // 2
    d64, x64 = dy.detach().double().cpu(), x.detach().double().cpu()
    return _conv_weight(x64, tuple(w_shape), d64, p), _conv_weight(x64.abs(), tuple(w_shape), d64.abs(), p).float()


# ---------------------------------------------------------------------------- the same references as plain sums over taps
def _taps(nd, K):
    return itertools.product(range(K), repeat=nd)


def _pad(t, h):
    return F.pad(t, (h, h) * (t.dim() - 2))


def _shifted(tp, k, sp):
    """[B, C, S] copy of the view of tp (padded by h) that starts at offset k: element pos is tp[pos + k] = t[pos + k - h]."""
    v = tp[(slice(None), slice(None)) + tuple(slice(a, a + n) for a, n in zip(k, sp))]
    return v.reshape(tp.shape[0], tp.shape[1], -1)


def _tap(w, k):
    return w[(slice(None), slice(None)) + tuple(k)]


def fwd_taps(x64, w64, halo=None):
    """sum over taps; halo < K // 2 is the seeded defect of a kernel that stages too narrow a halo: a tap further than
    `halo` from the centre along any axis finds nothing staged and reads zero."""
    K, sp = side(w64.shape), tuple(x64.shape[2:])
    h = K // 2
    xp = _pad(x64, h)
    y = torch.zeros(x64.shape[0], w64.shape[0], x64[0, 0].numel(), dtype=torch.float64)
    for k in _taps(len(sp), K):
        if halo is not None and any(abs(a - h) > halo for a in k):
            continue
        y += torch.einsum("oc,bcs->bos", _tap(w64, k), _shifted(xp, k, sp))
    return y.reshape((x64.shape[0], w64.shape[0]) + sp)


def bwd_data_taps(dy64, w64, reverse=True):
    """reverse=False: the seeded defect of a flip that swaps the channel roles but forgets to reverse the taps."""
    K, sp = side(w64.shape), tuple(dy64.shape[2:])
    h = K // 2
    dp = _pad(dy64, h)
    dx = torch.zeros(dy64.shape[0], w64.shape[1], dy64[0, 0].numel(), dtype=torch.float64)
    for k in _taps(len(sp), K):
        # y[pos] takes w[k] x[pos + k - h], so x[q] gives w[k] to y[q - k + h]: dy's view at offset 2h - k
        off = tuple(2 * h - a for a in k) if reverse else k
        dx += torch.einsum("oc,bos->bcs", _tap(w64, k), _shifted(dp, off, sp))
    return dx.reshape((dy64.shape[0], w64.shape[1]) + sp)


def bwd_weight_taps(dy64, x64, K):
    sp = tuple(dy64.shape[2:])
    xp = _pad(x64, K // 2)
    d = dy64.reshape(dy64.shape[0], dy64.shape[1], -1)
    dw = torch.empty((dy64.shape[1], x64.shape[1]) + (K,) * len(sp), dtype=torch.float64)
    for k in _taps(len(sp), K):
        dw[(slice(None), slice(None)) + tuple(k)] = torch.einsum("bos,bcs->oc", d, _shifted(xp, k, sp))
    return dw


# ------------------------------------------------------------------------------------------------------------ test inputs
def shape_of(B, C, T, H, W, dims):
    return (B, C, T, H, W) if dims == 3 else (B, C, H, W)


def make_case(case, K, dims, seed=0):
    """(x, w, b, dy) on the CPU, fp32, for case = (B, Cin, Cout, T, H, W) (T ignored -> 1 for dims == 2)."""
    B, Ci, Co, T, H, W = case
    if dims == 2:
        T = 1
    g = torch.Generator().manual_seed(1000 * K + 10 * dims + seed + 7 * (Ci + 31 * Co + H + 17 * W))
    x = torch.rand(shape_of(B, Ci, T, H, W, dims), generator=g) * 2 - 1
    w = (torch.rand((Co, Ci) + (K,) * dims, generator=g) * 2 - 1) / (Ci * K ** dims) ** 0.5
    b = torch.rand(Co, generator=g) - 0.5
    dy = torch.rand(shape_of(B, Co, T, H, W, dims), generator=g) * 2 - 1
    return x, w, b, dy


def geo(x_shape, Cin, Cout, K):
    """(B, Cin, Cout, T, H, W, KT, K) of the C ABI for an activation of x_shape (2-D: T = 1, KT = 1)."""
    if len(x_shape) == 5:
        B, _, T, H, W = x_shape
        return B, Cin, Cout, T, H, W, K, K
    B, _, H, W = x_shape
    return B, Cin, Cout, 1, H, W, 1, K
