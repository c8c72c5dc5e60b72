"""torch.autograd.Function wrappers over the C ABI (include/hpvg.h).

torch is used for device memory, streams and graph bookkeeping only; every arithmetic kernel below is a
hand-written gfx950 kernel in libhpvg.so.  The convolution family {Conv, ConvBwdData, ConvBwdWeight,
LReLUMaskMul} is closed under differentiation (each backward is expressed with the other Functions), which is
what the WGAN-GP double backward through the discriminator needs (reference: modules/utils.py:14-18)."""
import collections
import ctypes
import os

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .lib import PACK_BATCH_MAX, SN_BATCH_MAX, call, load, ptr, stream

_ws_cache = {}
_kernel_timer = None


class KernelTimer:
    """Brackets matching conv launches with HIP events recorded on the launch stream (torch's current stream is the
    stream every kernel of this package is enqueued on), so bench.py can report the dominant kernel's average
    duration measured live inside its timed region."""

    def __init__(self, match):
        """match(desc) -> a family name (str) for launches to time, else None.  desc: {"op": "conv" | "wgrad", "Cin", "Cout",
        "KT", and for convs "flip", "var"} in the kernel's view; launches of the tap-generic family (5 or 7 taps per axis)
        also carry "K", the tap side."""
        self.match = match
        self.events = []

    def begin(self, desc):
        fam = self.match(desc)
        if not fam:
            return None
        e0 = torch.cuda.Event(enable_timing=True)
        e0.record()
        return (fam, e0)

    def end(self, tok, key):
        if tok is None:
            return
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record()
        self.events.append(((tok[0],) + tuple(key), tok[1], e1))

    def summary(self):
        """{(family, B, Cin, Cout, T, H, W): (average ms, launches)} - call after a device synchronise."""
        acc = {}
        for key, e0, e1 in self.events:
            ms = e0.elapsed_time(e1)
            tot, n = acc.get(key, (0.0, 0))
            acc[key] = (tot + ms, n + 1)
        return {k: (tot / n, n) for k, (tot, n) in acc.items()}


def set_kernel_timer(t):
    global _kernel_timer
    _kernel_timer = t


_ws_pinned = []


def pin_workspaces():
    """From now on a scratch buffer that is outgrown is kept alive instead of freed: a captured hipGraph holds the raw
    address of the buffer that was current at capture time, and replays it long after a larger stage replaced it."""
    if not _ws_pinned:
        _ws_pinned.append(None)
    _ws_pinned.extend(_ws_cache.values())


def workspace(nbytes, device):
    """Stream-ordered scratch buffer shared by all ops on `device` (grown on demand)."""
    key = (device.type, device.index)
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
        _ws_cache[key] = buf
        if _ws_pinned:
            _ws_pinned.append(buf)
    return buf


def _scratch(nbytes, device):
    """The launch arguments (pointer, size) of the shared scratch buffer, grown to `nbytes`; the size is the buffer's own."""
    ws = workspace(nbytes, device)
    return ptr(ws), ws.numel()


def _c(t):
    return t if t.is_contiguous() else t.contiguous()


def geom(x):
    """(B, C, T, H, W) of an NCDHW / NCHW activation."""
    if x.dim() == 5:
        B, C, T, H, W = x.shape
    elif x.dim() == 4:
        B, C, H, W = x.shape
        T = 1
    else:
        raise RuntimeError("expected a 4-D or 5-D activation, got %s" % (tuple(x.shape),))
    return B, C, T, H, W


TAP_SIDES = (3, 5, 7)    # 3: the tuned family (hpvg_conv_*); 5 and 7: the tap-generic family (hpvg_convk_*)


def _side(w_shape):
    """Tap side K of a cubic conv weight [Co][Ci][K][K](, [K]); anything but a cube of side 3, 5 or 7 is refused."""
    nd = len(w_shape) - 2
    if nd not in (2, 3):
        raise RuntimeError("bad weight shape %s" % (tuple(w_shape),))
    k = int(w_shape[2])
    if tuple(w_shape[2:]) != (k,) * nd or k not in TAP_SIDES:
        raise RuntimeError("only %s kernels with K in {3, 5, 7} are supported on the MI355X path, got %s" % (
            "KxKxK" if nd == 3 else "KxK", tuple(w_shape),))
    return k


def _kt(w_shape):
    """KT of the C ABI: the tap side for 3-D weights, 1 for 2-D."""
    k = _side(w_shape)
    return k if len(w_shape) == 5 else 1


# ------------------------------------------------------------------------------------------ raw launches
_pack_cache = {}


def weights_changed():
    """Forget every packed weight: called by whatever rewrites parameters behind torch's back (the Adam kernel writes
    through raw pointers, so no version counter moves) and around hipGraph capture."""
    _pack_cache.clear()


def _wants_2d(geom_k, cin_k, cout_k, KT):
    """Does a launch of this geometry read the pack's two-axis Winograd section?  (lib query; negative results are the
    common case and decide nothing else)"""
    if geom_k is None or KT != 3:
        return None if geom_k is None else False
    B, T, H, W = geom_k
    return load().hpvg_conv_wants_wino2d(B, cin_k, cout_k, T, H, W, KT) == 1


def pack_weight(w, flip, geom_k=None):
    """Natural [Co][Ci][taps] weight -> MFMA fragment order (forward, or backward-data when flip).

    The same weight is packed for several launches between two optimizer steps (rec and rand generator passes; forward,
    backward-data and the double-backward convs of one discriminator evaluation): the packed copy is kept until
    `weights_changed()`, keyed by the weight's storage and validated by its version counter.  The entry holds a
    detached alias of the weight, so the allocator cannot hand the address to another tensor while the entry lives.
    geom_k = (B, T, H, W) of the launch that will read the pack: the two-axis Winograd fragments (the largest section)
    are then only written when that launch runs the two-axis kernel; without it the pack serves every launch."""
    w = _c(w)
    Co, Ci = w.shape[0], w.shape[1]
    KT = _kt(w.shape)
    if _side(w.shape) != 3:
        return w      # the tap-generic launches take the natural layout (they pack into their workspace per launch)
    cin_k, cout_k = (Co, Ci) if flip else (Ci, Co)
    has2d = _wants_2d(geom_k, cin_k, cout_k, KT)
    key = (w.data_ptr(), bool(flip), tuple(w.shape))
    hit = _pack_cache.get(key)
    # (an entry packed with the section serves a launch that does not need it; None = packed without a geometry = all sections)
    if hit is not None and hit[0] == w._version and hit[1].device == w.device and (hit[3] is None or hit[3] is True or has2d is False):
        return hit[2]
    if geom_k is None:
        n = call("hpvg_conv_wpack_floats", cin_k, cout_k, KT)
        wp = torch.empty(n, dtype=torch.float32, device=w.device)
        call("hpvg_conv_pack_weight_f32", ptr(w), None, ptr(wp), Ci, Co, KT, 1 if flip else 0, stream())
    else:
        B, T, H, W = geom_k
        n = call("hpvg_conv_wpack_floats_for", cin_k, cout_k, KT, B, T, H, W)
        wp = torch.empty(n, dtype=torch.float32, device=w.device)
        call("hpvg_conv_pack_weight_for_f32", ptr(w), None, ptr(wp), Ci, Co, KT, 1 if flip else 0, B, T, H, W, stream())
    _pack_cache[key] = (w._version, w.detach(), wp, has2d)
    return wp


def prepack_weights(ws, flips=(False, True), geom_k=None):
    """Pack several weights of one square layer shape (C -> C, C > 4) in ONE launch and leave the results in the pack cache,
    where the convs that follow find them (a discriminator forward packs its six spectral-norm weights twice each - forward
    and backward-data - which used to be a dozen 4.5 us launches in a row).  Weights of other shapes are left to
    pack_weight.  geom_k = (B, T, H, W) of the launches that will read them (see pack_weight)."""
    items = []
    for w in ws:
        if w.dim() < 4 or w.shape[0] != w.shape[1] or w.shape[0] <= 4 or not w.is_contiguous() or _side(w.shape) != 3:
            continue
        for f in flips:
            key = (w.data_ptr(), bool(f), tuple(w.shape))
            hit = _pack_cache.get(key)
            if hit is None or hit[0] != w._version:
                items.append((w, bool(f), key))
    if not items:
        return
    shape = tuple(items[0][0].shape)
    items = [it for it in items if tuple(it[0].shape) == shape][:PACK_BATCH_MAX]
    C, KT = shape[0], _kt(shape)
    has2d = _wants_2d(geom_k, C, C, KT)
    if geom_k is None:
        nfl = call("hpvg_conv_wpack_floats", C, C, KT)
    else:
        nfl = call("hpvg_conv_wpack_floats_for", C, C, KT, *geom_k)
    dev = items[0][0].device
    wps = [torch.empty(nfl, dtype=torch.float32, device=dev) for _ in items]
    m = len(items)
    PA, IA = ctypes.c_void_p * m, ctypes.c_int * m
    if geom_k is None:
        call("hpvg_conv_pack_weight_batch_f32", m, PA(*[ptr(it[0]) for it in items]), PA(*[ptr(t) for t in wps]),
             IA(*[1 if it[1] else 0 for it in items]), C, KT, stream())
    else:
        call("hpvg_conv_pack_weight_batch_for_f32", m, PA(*[ptr(it[0]) for it in items]), PA(*[ptr(t) for t in wps]),
             IA(*[1 if it[1] else 0 for it in items]), C, KT, *geom_k, stream())
    for (w, f, key), wp in zip(items, wps):
        _pack_cache[key] = (w._version, w.detach(), wp, has2d)


def conv_fwd_raw(x, w, bias, out_lrelu=False, flip=False, in_affine=None, in_lrelu=False, out_mask=None, mask_bits=None,
                 want_bits=False):
    """y = conv(f(x), w) (+bias); flip=True runs the backward-data conv of the layer weight w.
    out_mask (shaped like y): y *= (out_mask > 0 ? 1 : 0.2) in the kernel's epilogue (leaky_relu_backward of the layer below);
    mask_bits: the same mask in 1-bit form (int32 words, written by the producer of the activation: want_bits=True with
    out_lrelu returns (y, bits))."""
    x = _c(x)
    B, C, T, H, W = geom(x)
    KT = _kt(w.shape)
    Co_l, Ci_l = w.shape[0], w.shape[1]
    cin_k, cout_k = (Co_l, Ci_l) if flip else (Ci_l, Co_l)
    if C != cin_k:
        raise RuntimeError("conv: input has %d channels, weight expects %d" % (C, cin_k))
    shape = (B, cout_k, T, H, W) if x.dim() == 5 else (B, cout_k, H, W)
    K = _side(w.shape)
    if K != 3:
        # the tap-generic family: natural-layout weight, fp32 out_mask only (no 1-bit mask forms, no BatchNorm prologue)
        if in_affine is not None or in_lrelu:
            raise NotImplementedError("conv: the fused BatchNorm prologue exists for 3-tap weights only")
        if (x.dim() == 5) != (w.dim() == 5):
            raise RuntimeError("conv: a %d-D activation with a %d-D weight" % (x.dim(), w.dim()))
        if mask_bits is not None and out_mask is None:
            raise RuntimeError("conv: a %d-tap conv takes the fp32 out_mask, not mask_bits" % K)
        if out_mask is not None and tuple(out_mask.shape) != tuple(shape):
            raise RuntimeError("conv: out_mask has shape %s, the output %s" % (tuple(out_mask.shape), tuple(shape)))
        y = torch.empty(shape, dtype=torch.float32, device=x.device)
        timed = None
        if _kernel_timer is not None:
            timed = _kernel_timer.begin({"op": "conv", "Cin": cin_k, "Cout": cout_k, "KT": KT, "K": K, "flip": flip,
                                         "var": "mask" if out_mask is not None else "plain"})
        ws = _scratch(call("hpvg_convk_fwd_ws_bytes", B, cin_k, cout_k, T, H, W, KT, K), x.device)
        call("hpvg_convk_fwd_f32", ptr(x), ptr(_c(w)), ptr(bias), ptr(y), 1 if out_lrelu else 0,
             ptr(_c(out_mask)) if out_mask is not None else None, 1 if flip else 0, *ws, B, cin_k, cout_k, T, H, W, KT, K, stream())
        if timed is not None:
            _kernel_timer.end(timed, (B, cin_k, cout_k, T, H, W))
        return (y, None) if want_bits else y
    wp = pack_weight(w, flip, (B, T, H, W))
    y = torch.empty(shape, dtype=torch.float32, device=x.device)
    sc = sh = None
    if in_affine is not None:
        sc, sh = in_affine
    timed = None
    if _kernel_timer is not None:
        var = "pro" if in_affine is not None else ("mask" if (out_mask is not None or mask_bits is not None) else ("bits" if want_bits else "plain"))
        timed = _kernel_timer.begin({"op": "conv", "Cin": cin_k, "Cout": cout_k, "KT": KT, "flip": flip, "var": var})
    nws = call("hpvg_conv_fwd_ws_bytes", B, cin_k, cout_k, T, H, W, KT)
    ws = _scratch(nws, x.device) if nws else (None, 0)   # no workspace: NULL, 0 (one workgroup per tile)
    if out_mask is not None and tuple(out_mask.shape) != tuple(shape):
        raise RuntimeError("conv: out_mask has shape %s, the output %s" % (tuple(out_mask.shape), tuple(shape)))
    bits = None
    if (mask_bits is not None or want_bits) and cout_k > 4 and in_affine is None:
        if want_bits:
            bits = torch.empty(call("hpvg_conv_mask_words", B, cout_k, T, H, W), dtype=torch.int32, device=x.device)
        if mask_bits is not None and mask_bits.numel() != call("hpvg_conv_mask_words", B, cout_k, T, H, W):
            raise RuntimeError("conv: mask_bits has %d words, the output needs %d" % (mask_bits.numel(), call("hpvg_conv_mask_words", B, cout_k, T, H, W)))
        call("hpvg_conv_fwd_bits_f32", ptr(x), ptr(wp), ptr(bias), ptr(y), 1 if out_lrelu else 0, ptr(mask_bits), ptr(bits), *ws,
             B, cin_k, cout_k, T, H, W, KT, stream())
    else:
        call("hpvg_conv_fwd_f32", ptr(x), ptr(wp), ptr(bias), ptr(sc), ptr(sh), 1 if in_lrelu else 0, ptr(y),
             1 if out_lrelu else 0, ptr(_c(out_mask)) if out_mask is not None else None, *ws, B, cin_k, cout_k, T, H, W, KT, stream())
    if timed is not None:
        _kernel_timer.end(timed, (B, cin_k, cout_k, T, H, W))
    return (y, bits) if want_bits else y


_DIRECT_GRAD = os.environ.get("HPVG_DIRECT_GRAD", "1") != "0"


def grad_slot(p):
    """The gradient buffer of parameter `p` when a backward kernel may add its result straight into it, else None.

    autograd would take the returned gradient and run `p.grad += it` as one more (4.7 us) kernel per parameter and
    contribution - ~210 per GAN iteration.  The kernels that produce parameter gradients (weight-gradient reduce, channel
    sum, BatchNorm finalize, spectral-norm backward) can do that addition themselves: when `p` is a leaf that already has
    a dense fp32 `.grad` (the trainers' ParamArena gives every parameter one, zeroed per step) and no graph is being
    recorded, the Function adds into `p.grad` and returns None for that input.  Same numbers as AccumulateGrad;
    tensor hooks on `p` do not fire for it (HPVG_DIRECT_GRAD=0 restores plain autograd accumulation)."""
    if not _DIRECT_GRAD or p is None or torch.is_grad_enabled() or not (p.is_leaf and p.requires_grad):
        return None
    g = p.grad
    if g is None or g.dtype != torch.float32 or g.shape != p.shape or g.device != p.device or not g.is_contiguous():
        return None
    return g


def conv_bwd_weight_raw(dy, x, w_shape, into=None):
    """dw of the conv; `into` (a gradient buffer of the weight's shape): add the result into it and return None."""
    dy = _c(dy)
    x = _c(x)
    B, Co, T, H, W = geom(dy)
    Ci = x.shape[1]
    KT = _kt(w_shape)
    if (Co, Ci) != (w_shape[0], w_shape[1]):
        raise RuntimeError("conv_bwd_weight: channel mismatch")
    K = _side(w_shape)
    if K != 3:
        if (dy.dim() == 5) != (len(w_shape) == 5) or tuple(x.shape[2:]) != tuple(dy.shape[2:]) or x.shape[0] != B:
            raise RuntimeError("conv_bwd_weight: dy %s, x %s, weight %s" % (tuple(dy.shape), tuple(x.shape), tuple(w_shape)))
        ws = _scratch(call("hpvg_convk_bwd_weight_ws_bytes", B, Ci, Co, T, H, W, KT, K), dy.device)
        dw = into if into is not None else torch.empty(tuple(w_shape), dtype=torch.float32, device=dy.device)
        timed = _kernel_timer.begin({"op": "wgrad", "Cin": Ci, "Cout": Co, "KT": KT, "K": K, "bias": False}) if _kernel_timer is not None else None
        call("hpvg_convk_bwd_weight_f32", ptr(dy), ptr(x), ptr(dw), 1 if into is not None else 0, *ws, B, Ci, Co, T, H, W, KT, K, stream())
        if timed is not None:
            _kernel_timer.end(timed, (B, Ci, Co, T, H, W))
        return None if into is not None else dw
    ws = _scratch(call("hpvg_conv_bwd_weight_ws_bytes", B, Ci, Co, T, H, W, KT), dy.device)
    dw = into if into is not None else torch.empty(tuple(w_shape), dtype=torch.float32, device=dy.device)
    timed = _kernel_timer.begin({"op": "wgrad", "Cin": Ci, "Cout": Co, "KT": KT, "bias": False}) if _kernel_timer is not None else None
    call("hpvg_conv_bwd_weight_f32", ptr(dy), ptr(x), None, None, 0, ptr(dw), 1 if into is not None else 0, *ws, B, Ci, Co, T, H, W, KT,
         stream())
    if timed is not None:
        _kernel_timer.end(timed, (B, Ci, Co, T, H, W))
    return None if into is not None else dw


def conv_bwd_weight_bias_raw(dy, x, w_shape, into_w, into_b):
    """dw AND the bias gradient from one launch where the library can (wide layers on the Winograd weight-gradient kernel),
    both added into their gradient buffers; returns False when the layer is not one of those (nothing was launched)."""
    dy = _c(dy)
    x = _c(x)
    B, Co, T, H, W = geom(dy)
    Ci = x.shape[1]
    KT = _kt(w_shape)
    if _side(w_shape) != 3 or load().hpvg_conv_bwd_weight_fuses_bias(B, Ci, Co, T, H, W, KT) != 1:
        return False
    ws = _scratch(call("hpvg_conv_bwd_weight_ws_bytes", B, Ci, Co, T, H, W, KT), dy.device)
    timed = _kernel_timer.begin({"op": "wgrad", "Cin": Ci, "Cout": Co, "KT": KT, "bias": True}) if _kernel_timer is not None else None
    call("hpvg_conv_bwd_weight_bias_f32", ptr(dy), ptr(x), ptr(into_w), 1, ptr(into_b), 1, *ws, B, Ci, Co, T, H, W, KT, stream())
    if timed is not None:
        _kernel_timer.end(timed, (B, Ci, Co, T, H, W))
    return True


def channel_sum_raw(dy, into=None):
    dy = _c(dy)
    B, C, T, H, W = geom(dy)
    out = into if into is not None else torch.empty(C, dtype=torch.float32, device=dy.device)
    call("hpvg_channel_sum_f32", ptr(dy), ptr(out), 1 if into is not None else 0,
         *_scratch(call("hpvg_channel_sum_ws_bytes", C), dy.device), B, C, T * H * W, stream())
    return None if into is not None else out


def _weight_grad(dy, x, w):
    """dw for Conv / ConvBwdData backward: added straight into w.grad when allowed (returns None), else a Function."""
    slot = grad_slot(w)
    if slot is not None:
        return conv_bwd_weight_raw(dy, x, w.shape, into=slot)
    return ConvBwdWeight.apply(dy, x, w.shape)


def _scalar_out(device):
    return torch.empty(1, dtype=torch.float32, device=device)


def _reduce_ws(device):
    """The launch arguments (pointer, size) of the reductions' scratch."""
    n = call("hpvg_reduce_ws_bytes")
    return ptr(workspace(n, device)), n


class inputs_only:
    """with ops.inputs_only(): a backward pass that is known to want gradients w.r.t. activations only
    (torch.autograd.grad(D(x_hat), x_hat) of the gradient penalty).  A Python autograd Function cannot see which of its
    inputs the running graph task needs - ctx.needs_input_grad only says "requires grad" - so without this every conv
    of the critic would also launch its weight- and bias-gradient kernels there, for results the engine throws away."""
    active = False

    def __enter__(self):
        self.prev = inputs_only.active
        inputs_only.active = True

    def __exit__(self, *exc):
        inputs_only.active = self.prev


# ------------------------------------------------------------------------------------------ conv family
# Conv.backward hands the LeakyReLU mask operands (activations of the forward pass) to ConvBwdData / LReLUMaskMul.  Under
# create_graph=True (the gradient penalty) an operand that requires grad gives the new node an edge to the forward Conv
# that produced it; no gradient is ever returned along it (LeakyReLU's second derivative is zero), but the engine still
# runs that producer - on a materialised tensor of zeros - when the penalty is back-propagated: a whole backward pass of
# D(x_hat) for nothing.  Detached operands carry the same values and no edge.  Not a user flag: the tests run both forms.
DETACH_MASKS = True


class LReLUMaskMul(Function):
    """dy * (h > 0 ? 1 : 0.2) - leaky_relu_backward on the activated tensor (reference: networks_3d.py:21)."""

    @staticmethod
    def forward(ctx, dy, h):
        dy = _c(dy)
        out = torch.empty_like(dy)
        call("hpvg_lrelu_mask_mul_f32", ptr(dy), ptr(h), ptr(out), dy.numel(), stream())
        ctx.save_for_backward(h)
        return out

    @staticmethod
    def backward(ctx, g):
        (h,) = ctx.saved_tensors
        return LReLUMaskMul.apply(g, h), None


class ChannelSum(Function):
    @staticmethod
    def forward(ctx, dy):
        ctx.shape = dy.shape
        return channel_sum_raw(dy)

    @staticmethod
    def backward(ctx, g):
        view = [1, -1] + [1] * (len(ctx.shape) - 2)
        return g.view(*view).expand(ctx.shape).contiguous()


class Conv(Function):
    """y = conv3x3(x, w) + b, optionally followed by LeakyReLU(0.2) (ConvBlock3DSN / plain tails).

    Chains of activated convs (the spectral-norm critic and encoder: networks_3d.py:59-70,163-181) hand the LeakyReLU's
    backward mask from the PRODUCER of an activation to its CONSUMER, where it costs nothing: the consumer's backward-data
    conv computes the gradient w.r.t. the activated tensor - its own saved input - and multiplies by the mask in its
    epilogue (conv_fwd_raw(out_mask=)); leaky_relu_backward as a pass of its own (three tensor sweeps per layer and
    backward chain) is gone.
      in_act       : x is the output of a Conv(act=True, out_masked_by_consumer=True): dx is masked with lrelu'(x) here
      mask_by_consumer : (with act) every consumer of y is such a Conv, so this backward must NOT mask dy again."""

    @staticmethod
    def forward(ctx, x, w, b, act, in_act=False, mask_by_consumer=False, in_bits=None):
        """in_bits: the 1-bit LeakyReLU mask of x as its producer's epilogue wrote it (see Conv.apply_bits); the
        backward-data epilogue then reads 1/32 of the bytes.  Without it (row slabs: x was extended by halo rows) the mask
        is read from x itself."""
        want = act and mask_by_consumer and w.shape[0] > 4
        if want:
            y, bits = conv_fwd_raw(x, w, b, out_lrelu=True, want_bits=True)
            Conv.last_bits = bits          # handed to the caller by apply_bits (not an autograd output)
        else:
            y = conv_fwd_raw(x, w, b, out_lrelu=act)
            Conv.last_bits = None
        own_mask = act and not mask_by_consumer
        ctx.save_for_backward(x, w, y if own_mask else None, b, in_bits if in_act else None)
        ctx.own_mask, ctx.in_act = own_mask, in_act
        ctx.has_bias = b is not None
        return y

    last_bits = None

    @staticmethod
    def apply_bits(x, w, b, act, in_act=False, mask_by_consumer=False, in_bits=None):
        """Conv.apply that also returns the 1-bit mask of the activated output (None when this call made none)."""
        y = Conv.apply(x, w, b, act, in_act, mask_by_consumer, in_bits)
        bits, Conv.last_bits = Conv.last_bits, None
        return y, bits

    @staticmethod
    def backward(ctx, dy):
        x, w, y, b, in_bits = ctx.saved_tensors
        dy = _c(dy)
        if DETACH_MASKS:
            x_mask, y_mask = x.detach(), (y.detach() if y is not None else None)
        else:
            x_mask, y_mask = x, y
        if ctx.own_mask:
            dy = LReLUMaskMul.apply(dy, y_mask)
        params = not inputs_only.active
        dx = ConvBwdData.apply(dy, w, x_mask if ctx.in_act else None, in_bits) if ctx.needs_input_grad[0] else None
        want_w = ctx.needs_input_grad[1] and params
        want_b = ctx.has_bias and ctx.needs_input_grad[2] and params
        if want_w and want_b:
            # both straight into their gradient buffers from ONE launch where the library fuses them
            ws_, bs_ = grad_slot(w), grad_slot(b)
            if ws_ is not None and bs_ is not None and conv_bwd_weight_bias_raw(dy, x, w.shape, ws_, bs_):
                return dx, None, None, None, None, None, None
        dw = _weight_grad(dy, x, w) if want_w else None
        db = None
        if want_b:
            slot = grad_slot(b)
            db = channel_sum_raw(dy, into=slot) if slot is not None else ChannelSum.apply(dy)
        return dx, dw, db, None, None, None, None


class ConvBwdData(Function):
    """dx = conv(dy, flip/transpose(w)) [* lrelu'(h)]: backward-data of a stride-1 'same' conv; with h (the activated tensor
    the conv consumed) the LeakyReLU backward of the layer below is applied in the kernel's epilogue - from the 1-bit mask
    `bits` when the producer of h wrote one."""

    @staticmethod
    def forward(ctx, dy, w, h=None, bits=None):
        ctx.save_for_backward(dy, w, h)
        if h is not None and bits is not None and w.shape[1] > 4:
            return conv_fwd_raw(dy, w, None, flip=True, mask_bits=bits)
        return conv_fwd_raw(dy, w, None, flip=True, out_mask=h)

    @staticmethod
    def backward(ctx, g):
        dy, w, h = ctx.saved_tensors
        g = _c(g)
        if h is not None:
            g = LReLUMaskMul.apply(g, h)     # second order only (the gradient penalty's double backward): a pass of its own
        ddy = Conv.apply(g, w, None, False) if ctx.needs_input_grad[0] else None
        dw = _weight_grad(dy, g, w) if ctx.needs_input_grad[1] else None
        return ddy, dw, None, None


class ConvBwdWeight(Function):
    """dw[o][c][tap] = sum dy[o][n] * x[c][n + off(tap)]."""

    @staticmethod
    def forward(ctx, dy, x, w_shape):
        ctx.save_for_backward(dy, x)
        return conv_bwd_weight_raw(dy, x, w_shape)

    @staticmethod
    def backward(ctx, gw):
        dy, x = ctx.saved_tensors
        gw = _c(gw)
        ddy = Conv.apply(x, gw, None, False) if ctx.needs_input_grad[0] else None
        dx = ConvBwdData.apply(dy, gw) if ctx.needs_input_grad[1] else None
        return ddy, dx, None


# ------------------------------------------------------------------------------------------ BatchNorm + LeakyReLU
class BNAct(Function):
    """h = LeakyReLU_opt(BatchNorm_train(r)) with running-stat update (ConvBlock3D: networks_3d.py:54-56).

    groups > 1: the batch holds `groups` independent passes of the network one after the other (the merged rec + rand
    generator pass, GeneratorHPVAEGAN.forward_pair); every group is normalised with ITS OWN batch statistics and the
    running statistics are updated once per group, in order - exactly what the separate passes would do (the kernels take
    the group count: one launch pair for all groups)."""

    @staticmethod
    def forward(ctx, r, gamma, beta, running_mean, running_var, momentum, eps, lrelu, groups=1):
        r = _c(r)
        B, C, T, H, W = geom(r)
        S = T * H * W
        dev = r.device
        assert B % groups == 0
        stats = torch.empty(groups, 4, C, dtype=torch.float32, device=dev)  # per group: mean, invstd, scale, shift
        nws = call("hpvg_bn_ws_bytes", C * groups)
        ws = _scratch(nws, dev)
        h = torch.empty_like(r)
        st = stats[0]
        call("hpvg_bn_train_fwd_f32", ptr(r), ptr(gamma), ptr(beta), ptr(running_mean), ptr(running_var),
             float(momentum), float(eps), ptr(st[0]), ptr(st[1]), ptr(st[2]), ptr(st[3]), ptr(h),
             1 if lrelu else 0, groups, *ws, B, C, S, stream())
        ctx.save_for_backward(r, stats, gamma, beta)
        ctx.lrelu, ctx.groups = lrelu, groups
        return h

    @staticmethod
    def backward(ctx, dh):
        r, stats, gamma, beta = ctx.saved_tensors
        dh = _c(dh)
        if torch.is_grad_enabled():
            # a graph is being recorded over this backward (create_graph=True: the gradient penalty of a critic that contains
            # BatchNorm, WDiscriminatorBaselines): run it as a differentiable op of its own
            if ctx.groups != 1:
                raise NotImplementedError("second-order BatchNorm is implemented for groups == 1")
            dr, dg, db = BNActBwd.apply(dh, r, gamma, stats, ctx.lrelu)
            return dr, dg, db, None, None, None, None, None, None
        B, C, T, H, W = geom(r)
        S = T * H * W
        dev = r.device
        groups = ctx.groups
        dr = torch.empty_like(r)
        sg, sb = grad_slot(gamma), grad_slot(beta)
        direct = sg is not None and sb is not None and ctx.needs_input_grad[1] and ctx.needs_input_grad[2]
        dgb = (sg, sb) if direct else torch.empty(2, C, dtype=torch.float32, device=dev)
        nws = call("hpvg_bn_ws_bytes", C * groups)
        ws = _scratch(nws, dev)
        st = stats[0]
        call("hpvg_bn_act_bwd_f32", ptr(dh), ptr(r), ptr(st[0]), ptr(st[1]), ptr(st[2]), ptr(st[3]),
             1 if ctx.lrelu else 0, groups, ptr(dr), ptr(dgb[0]), ptr(dgb[1]), 1 if direct else 0, *ws, B, C, S, stream())
        if direct:
            return dr, None, None, None, None, None, None, None, None
        return dr, dgb[0], dgb[1], None, None, None, None, None, None


class BNActBwd(Function):
    """(dr, dgamma, dbeta) = backward of BNAct as a DIFFERENTIABLE op: what BNAct.backward runs while a graph is recorded
    over it.  Its own backward is the second-order BatchNorm kernel pair (hpvg_bn_act_bwd2_f32): gradients w.r.t. dh, r and
    gamma of <dr, g>; dgamma / dbeta are not differentiated on the path (the penalty differentiates input gradients only)."""

    @staticmethod
    def forward(ctx, dh, r, gamma, stats, lrelu):
        B, C, T, H, W = geom(r)
        S = T * H * W
        dev = r.device
        dr = torch.empty_like(r)
        dgb = torch.empty(2, C, dtype=torch.float32, device=dev)
        ws = _scratch(call("hpvg_bn_ws_bytes", C), dev)
        st = stats[0]
        call("hpvg_bn_act_bwd_f32", ptr(dh), ptr(r), ptr(st[0]), ptr(st[1]), ptr(st[2]), ptr(st[3]), 1 if lrelu else 0, 1,
             ptr(dr), ptr(dgb[0]), ptr(dgb[1]), 0, *ws, B, C, S, stream())
        ctx.save_for_backward(dh, r, gamma, stats)
        ctx.lrelu = lrelu
        dg, db = dgb[0], dgb[1]
        ctx.mark_non_differentiable(dg, db)
        return dr, dg, db

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _g_dgamma, _g_dbeta):
        dh, r, gamma, stats = ctx.saved_tensors
        g = _c(g)
        B, C, T, H, W = geom(r)
        S = T * H * W
        dev = r.device
        g_dh = torch.empty_like(r) if ctx.needs_input_grad[0] else None
        g_r = torch.empty_like(r) if ctx.needs_input_grad[1] else None
        slot = grad_slot(gamma) if ctx.needs_input_grad[2] else None
        g_gamma = slot if slot is not None else (torch.empty(C, dtype=torch.float32, device=dev) if ctx.needs_input_grad[2] else None)
        ws = _scratch(call("hpvg_bn_bwd2_ws_bytes", C), dev)
        st = stats[0]
        call("hpvg_bn_act_bwd2_f32", ptr(dh), ptr(g), ptr(r), ptr(st[0]), ptr(st[1]), ptr(st[2]), ptr(st[3]), 1 if ctx.lrelu else 0,
             ptr(g_dh), ptr(g_r), ptr(g_gamma), 1 if slot is not None else 0, *ws, B, C, S, stream())
        return g_dh, g_r, (None if slot is not None else g_gamma), None, None


def concat_batch(parts, like=None):
    """torch.cat(parts, dim=0) for contiguous fp32 tensors of equal trailing shape, with kernel copies: torch.cat (and
    torch.zeros) may lower to hipMemcpyAsync / hipMemsetAsync, i.e. memcpy / memset NODES when the iteration is captured
    into a hipGraph, and those are not reliably ordered on this runtime.  An entry that is an int n
    stands for n zero samples."""
    ref = like if like is not None else next(p for p in parts if torch.is_tensor(p))
    tail = tuple(ref.shape[1:])
    per = 1
    for d in tail:
        per *= int(d)
    total = sum(p if isinstance(p, int) else p.shape[0] for p in parts)
    out = torch.empty((total,) + tail, dtype=torch.float32, device=ref.device)
    o = 0
    for p in parts:
        n = p if isinstance(p, int) else p.shape[0]
        src = None if isinstance(p, int) else ptr(_c(p.detach()))
        call("hpvg_copy_f32", src, ptr(out[o:o + n]), n * per, stream())
        o += n
    return out


class Concat2(Function):
    """Differentiable concat_batch of two tensors (the latent batch of the merged generator pass)."""

    @staticmethod
    def forward(ctx, a, b):
        ctx.n = a.shape[0]
        return concat_batch([a, b])

    @staticmethod
    def backward(ctx, g):
        g = _c(g)
        return g[:ctx.n], g[ctx.n:]


class SplitBatch(Function):
    """(x[:n], x[n:]) as two outputs.  torch's own slicing would do: but its backward builds the full-size gradient with
    at::zeros + copy, i.e. a hipMemsetAsync, which must not appear in an iteration that may be captured into a hipGraph
    (DESIGN.md section 4); this backward is one concatenation kernel."""

    @staticmethod
    def forward(ctx, x, n):
        x = _c(x)
        ctx.n, ctx.shape = n, x.shape
        return x[:n], x[n:]

    @staticmethod
    def backward(ctx, g0, g1):
        n, shape = ctx.n, ctx.shape
        if g0 is None and g1 is None:
            return None, None
        ref = g0 if g0 is not None else g1
        return concat_batch([g0 if g0 is not None else n, g1 if g1 is not None else shape[0] - n], like=ref), None


class BNActSync(Function):
    """BNAct with the batch split over the ranks of a process group (multi-GPU, one process per GPU): each rank reduces
    its own samples, `allreduce(t)` (a callable summing a float64 tensor over the group, in place) combines the
    per-channel pairs, and statistics / running buffers / dr follow from the global sums - the same arithmetic as BNAct
    over the whole batch.  dgamma / dbeta are this rank's share (the parameter all-reduce adds the shares up)."""

    @staticmethod
    def forward(ctx, r, gamma, beta, running_mean, running_var, momentum, eps, lrelu, allreduce, nranks, total=None):
        r = _c(r)
        B, C, T, H, W = geom(r)
        S = T * H * W
        dev = r.device
        ws = _scratch(call("hpvg_bn_ws_bytes", C), dev)
        sums = torch.empty(C, 2, dtype=torch.float64, device=dev)
        call("hpvg_bn_sums_f32", ptr(r), ptr(sums), *ws, B, C, S, stream())
        allreduce(sums)
        # elements per channel behind the statistics: `total` when the ranks hold unequal shares (row slabs)
        count = float(total) if total is not None else float(B) * float(S) * float(nranks)
        stats = torch.empty(4, C, dtype=torch.float32, device=dev)  # mean, invstd, scale, shift
        call("hpvg_bn_finalize_f32", ptr(sums), count, ptr(gamma), ptr(beta), ptr(running_mean), ptr(running_var),
             float(momentum), float(eps), ptr(stats[0]), ptr(stats[1]), ptr(stats[2]), ptr(stats[3]), C, stream())
        h = torch.empty_like(r)
        call("hpvg_affine_act_f32", ptr(r), ptr(stats[2]), ptr(stats[3]), ptr(h), 1 if lrelu else 0, B, C, S, stream())
        ctx.save_for_backward(r, stats)
        ctx.lrelu, ctx.allreduce, ctx.count = lrelu, allreduce, count
        return h

    @staticmethod
    @once_differentiable
    def backward(ctx, dh):
        r, stats = ctx.saved_tensors
        dh = _c(dh)
        B, C, T, H, W = geom(r)
        S = T * H * W
        dev = r.device
        ws = _scratch(call("hpvg_bn_ws_bytes", C), dev)
        local = torch.empty(C, 2, dtype=torch.float64, device=dev)  # (sum dz, sum dz*xhat) of this rank's samples
        call("hpvg_bn_act_bwd_sums_f32", ptr(dh), ptr(r), ptr(stats[0]), ptr(stats[1]), ptr(stats[2]), ptr(stats[3]),
             1 if ctx.lrelu else 0, ptr(local), *ws, B, C, S, stream())
        glob = local.clone()
        ctx.allreduce(glob)
        gsum = glob.to(torch.float32).contiguous()
        dr = torch.empty_like(r)
        call("hpvg_bn_act_bwd_apply_f32", ptr(dh), ptr(r), ptr(stats[0]), ptr(stats[1]), ptr(stats[2]), ptr(stats[3]),
             1 if ctx.lrelu else 0, ptr(gsum), float(1.0 / ctx.count), ptr(dr), B, C, S, stream())
        loc32 = local.to(torch.float32)
        return dr, loc32[:, 1].contiguous(), loc32[:, 0].contiguous(), None, None, None, None, None, None, None, None


class AffineAct(Function):
    """y = LeakyReLU_opt(scale[c]*x + shift[c]) - eval-mode BatchNorm apply (running statistics)."""

    @staticmethod
    def forward(ctx, r, scale, shift, lrelu):
        r = _c(r)
        B, C, T, H, W = geom(r)
        h = torch.empty_like(r)
        call("hpvg_affine_act_f32", ptr(r), ptr(_c(scale)), ptr(_c(shift)), ptr(h), 1 if lrelu else 0, B, C, T * H * W, stream())
        return h

    @staticmethod
    def backward(ctx, dh):
        raise NotImplementedError("eval-mode BatchNorm backward is not on the reference's train path")


# ------------------------------------------------------------------------------------------ spectral norm
class SpectralNormWeight(Function):
    """W = W_orig / sigma(W_orig), sigma = u^T W_mat v after one power iteration (u, v updated in place when
    training).  torch hook semantics: nn.utils.spectral_norm, n_power_iterations=1, eps=1e-12 (networks_3d.py:63)."""

    @staticmethod
    def forward(ctx, w_orig, u, v, do_iter, eps):
        w_orig = _c(w_orig)
        Co = w_orig.shape[0]
        K = w_orig.numel() // Co
        dev = w_orig.device
        sig = torch.empty(2, dtype=torch.float32, device=dev)  # sigma, 1/sigma
        ws = _scratch(Co * 4, dev)
        # later forwards overwrite the u/v buffers before this call's backward runs: the kernel also writes the (u, v) its
        # sigma belongs to into `uv` (torch clones them for the same reason); [0, Co) = u, [Co, Co + K) = v
        uv = torch.empty(Co + K, dtype=torch.float32, device=dev) if w_orig.requires_grad else None
        call("hpvg_sn_power_iter_f32", ptr(w_orig), ptr(u), ptr(v), ptr(sig[0:1]), ptr(sig[1:2]), ptr(uv), Co, K,
             1 if do_iter else 0, float(eps), *ws, stream())
        w = torch.empty_like(w_orig)
        call("hpvg_div_scalar_f32", ptr(w_orig), ptr(sig[0:1]), ptr(w), w.numel(), stream())
        ctx.save_for_backward(w_orig, uv, sig)
        return w

    @staticmethod
    @once_differentiable
    def backward(ctx, dw):
        w_orig, uv, sig = ctx.saved_tensors
        dw = _c(dw)
        Co = w_orig.shape[0]
        K = w_orig.numel() // Co
        slot = grad_slot(w_orig)
        out = slot if slot is not None else torch.empty_like(w_orig)
        ws = _scratch(call("hpvg_sn_bwd_ws_bytes", Co, K), dw.device)
        call("hpvg_sn_bwd_f32", ptr(dw), ptr(w_orig), ptr(uv[:Co]), ptr(uv[Co:]), ptr(sig[0:1]), ptr(out),
             1 if slot is not None else 0, *ws, Co, K, stream())
        return (None if slot is not None else out), None, None, None, None


class SpectralNormWeightBatch(Function):
    """SpectralNormWeight for up to 8 independent layers in ONE launch (one workgroup per layer: power iteration, sigma,
    the (u, v) copy for the backward and weight = weight_orig / sigma): the spectral-norm convs of a network all need
    their weight at the start of a forward, and six ~19 us single-workgroup launches in a row are pure latency.
    apply(do_iter, eps, w1, u1, v1, w2, u2, v2, ...) -> (weight1, weight2, ...).  The backward runs per layer (the
    gradients arrive layer by layer) with the same kernels as SpectralNormWeight."""

    @staticmethod
    def forward(ctx, do_iter, eps, *tensors):
        n = len(tensors) // 3
        assert 1 <= n <= SN_BATCH_MAX and len(tensors) == 3 * n
        ws_orig = [_c(tensors[3 * i]) for i in range(n)]
        us = [tensors[3 * i + 1] for i in range(n)]
        vs = [tensors[3 * i + 2] for i in range(n)]
        dev = ws_orig[0].device
        Cos = [w.shape[0] for w in ws_orig]
        Ks = [w.numel() // w.shape[0] for w in ws_orig]
        sig = torch.empty(n, 2, dtype=torch.float32, device=dev)
        need = [w.requires_grad for w in ws_orig]
        uvs = [torch.empty(Cos[i] + Ks[i], dtype=torch.float32, device=dev) if need[i] else None for i in range(n)]
        outs = [torch.empty_like(w) for w in ws_orig]
        ws = _scratch(4 * sum(Cos), dev)
        PA, IA = ctypes.c_void_p * n, ctypes.c_int * n
        call("hpvg_sn_power_iter_batch_f32", n, PA(*[ptr(w) for w in ws_orig]), PA(*[ptr(u) for u in us]), PA(*[ptr(v) for v in vs]),
             PA(*[ptr(sig[i]) for i in range(n)]), PA(*[ptr(t) for t in uvs]), PA(*[ptr(o) for o in outs]), IA(*Cos), IA(*Ks),
             1 if do_iter else 0, float(eps), *ws, stream())
        ctx.n = n
        ctx.save_for_backward(sig, *ws_orig, *uvs)
        return tuple(outs)

    @staticmethod
    @once_differentiable
    def backward(ctx, *dws):
        n = ctx.n
        saved = ctx.saved_tensors
        sig, ws_orig, uvs = saved[0], saved[1:1 + n], saved[1 + n:1 + 2 * n]
        grads = [None, None]
        live = [i for i in range(n) if dws[i] is not None and ctx.needs_input_grad[2 + 3 * i]]
        res = {}
        if live:
            m = len(live)
            dev = dws[live[0]].device
            dwc = [_c(dws[i]) for i in live]
            slots = [grad_slot(ws_orig[i]) for i in live]
            outs = [sl if sl is not None else torch.empty_like(ws_orig[i]) for sl, i in zip(slots, live)]
            Cos = [ws_orig[i].shape[0] for i in live]
            Ks = [ws_orig[i].numel() // ws_orig[i].shape[0] for i in live]
            ws = _scratch(sum(call("hpvg_sn_bwd_ws_bytes", c, k) for c, k in zip(Cos, Ks)), dev)
            PA, IA = ctypes.c_void_p * m, ctypes.c_int * m
            call("hpvg_sn_bwd_batch_f32", m, PA(*[ptr(t) for t in dwc]), PA(*[ptr(ws_orig[i]) for i in live]),
                 PA(*[ptr(uvs[i]) for i in live]), PA(*[ptr(sig[i, 0:1]) for i in live]), PA(*[ptr(o) for o in outs]),
                 IA(*[1 if sl is not None else 0 for sl in slots]), IA(*Cos), IA(*Ks), *ws, stream())
            for i, sl, o in zip(live, slots, outs):
                res[i] = None if sl is not None else o
        for i in range(n):
            grads += [res.get(i), None, None]
        return tuple(grads)


# ------------------------------------------------------------------------------------------ generator glue
class TanhRes(Function):
    """y = tanh(x + res)  (res optional): networks_3d.py:377 (vae_out) and :404 (residual refinement)."""

    @staticmethod
    def forward(ctx, x, res):
        x = _c(x)
        if res is not None:
            res = _c(res)
        y = torch.empty_like(x)
        call("hpvg_tanh_fwd_f32", ptr(x), ptr(res), ptr(y), x.numel(), stream())
        ctx.save_for_backward(y)
        ctx.has_res = res is not None
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        dy = _c(dy)
        dx = torch.empty_like(y)
        call("hpvg_tanh_bwd_f32", ptr(dy), ptr(y), ptr(dx), y.numel(), stream())
        return dx, (dx if ctx.has_res else None)


class Add(Function):
    """a + b: the pre-tanh residual of the SinGAN baseline (networks_3d.py:319)."""

    @staticmethod
    def forward(ctx, a, b):
        a, b = _c(a), _c(b)
        if a.shape != b.shape:
            raise RuntimeError("add: shape mismatch %s vs %s" % (tuple(a.shape), tuple(b.shape)))
        out = torch.empty_like(a)
        call("hpvg_add_f32", ptr(a), ptr(b), ptr(out), a.numel(), stream())
        return out

    @staticmethod
    def backward(ctx, g):
        return g, g


def _box_copy(src, grow):
    """[B, C, (T,) H, W] -> every spatial axis grown by 2 * grow (grow < 0 crops), src placed `grow` voxels in and the
    border zero (hpvg_box_copy_f32)."""
    src = _c(src)
    B, C, T, H, W = geom(src)
    oT = grow if src.dim() == 5 else 0
    dT, dH, dW = T + 2 * oT, H + 2 * grow, W + 2 * grow
    if min(dT, dH, dW) < 1:
        raise RuntimeError("crop of %d from %s leaves nothing" % (-grow, tuple(src.shape)))
    out = src.new_empty((B, C, dT, dH, dW) if src.dim() == 5 else (B, C, dH, dW))
    call("hpvg_box_copy_f32", ptr(src), ptr(out), B * C, T, H, W, dT, dH, dW, oT, grow, grow, stream())
    return out


class ZeroPad(Function):
    """F.pad(x, (p,) * 2 * spatial dims): the zero padding of the SinGAN baselines' volumes (networks_3d.py:205,247-268,
    300-318).  Its backward is CropBorder and CropBorder's is ZeroPad, so the pair is differentiable to any order (the
    critic's input pad sits inside the gradient penalty's double backward)."""

    @staticmethod
    def forward(ctx, x, p):
        ctx.p = p
        return _box_copy(x, p)

    @staticmethod
    def backward(ctx, g):
        return CropBorder.apply(g, ctx.p), None


class CropBorder(Function):
    """y[:, :, c:-c, c:-c(, c:-c)]: the outer `c`-voxel shell removed (a padding=0 convolution = the zero-padded one cropped
    by 1, _nets.crop_border).  Its backward is ZeroPad."""

    @staticmethod
    def forward(ctx, y, c=1):
        ctx.c = c
        return _box_copy(y, -c)

    @staticmethod
    def backward(ctx, g):
        return ZeroPad.apply(g, ctx.c), None


def _resize_out(ctx, x, size):
    """The empty output of a resize of x to `size`, and the kernels' (B * C, Ti, Hi, Wi, To, Ho, Wo), which ctx keeps with
    the input's shape for UpsampleAC.backward."""
    B, C, Ti, Hi, Wi = geom(x)
    To, Ho, Wo = size if x.dim() == 5 else (1,) + tuple(size)
    ctx.in_shape = x.shape
    ctx.dims = (B * C, Ti, Hi, Wi, To, Ho, Wo)
    return torch.empty((B, C) + tuple(size), dtype=torch.float32, device=x.device), ctx.dims


class UpsampleAC(Function):
    """Tri/bi-linear resize with align_corners=True to `size`; with `noise`, also returns up + amp*noise
    (utils/images.py:83-105 + networks_3d.py:395-400)."""

    @staticmethod
    def forward(ctx, x, size, noise, amp):
        x = _c(x)
        y, dims = _resize_out(ctx, x, size)
        yn = None
        if noise is not None:
            noise = _c(noise)
            if noise.shape != y.shape:
                raise RuntimeError("noise shape %s != upsampled shape %s" % (tuple(noise.shape), tuple(y.shape)))
            yn = torch.empty_like(y)
        call("hpvg_upsample_linear_ac_f32", ptr(x), ptr(y), ptr(noise), float(amp), ptr(yn), *dims, stream())
        if yn is None:
            return y
        return y, yn

    @staticmethod
    @once_differentiable
    def backward(ctx, dy, dyn=None):
        # both outputs (`up` and `up + amp*noise`) may carry a gradient: the kernel adds the two on load
        g, g2 = (dy, dyn) if dy is not None else (dyn, None)
        g = _c(g)
        g2 = _c(g2) if g2 is not None else None
        BC, Ti, Hi, Wi, To, Ho, Wo = ctx.dims
        dx = torch.empty(ctx.in_shape, dtype=torch.float32, device=g.device)
        call("hpvg_upsample_linear_ac_bwd_f32", ptr(g), ptr(g2), ptr(dx), BC, Ti, Hi, Wi, To, Ho, Wo, stream())
        return dx, None, None, None


# ------------------------------------------------------------------------------------------ rings (generate --wrap)
def _ring_input(x, what):
    """Rings are a sampling feature: no backward is built, so an input that would need one is refused."""
    if torch.is_grad_enabled() and x.requires_grad:
        raise RuntimeError("%s has no backward (rings are a sampling feature): run it under torch.no_grad()" % what)
    if x.dtype != torch.float32:
        raise RuntimeError("%s takes fp32, got %s" % (what, x.dtype))
    return _c(x)


def _per_axis(v, x, name, what):
    """One non-negative int per spatial axis of x as a triple (t, h, w); an image gets t = 0."""
    v = tuple(int(e) for e in v)
    if len(v) != x.dim() - 2 or min(v) < 0:
        raise ValueError("%s: %s must hold one value >= 0 per spatial axis of %s, got %r" % (what, name, tuple(x.shape), v))
    return v if x.dim() == 5 else (0,) + v


def ring_pad(x, pad):
    """[B, C, (T,) H, W] -> every spatial axis a grown by 2 * pad[a], filled circularly: out[.., i, ..] = x[.., (i - pad[a]) mod
    side, ..] (hpvg_ring_pad_f32).  pad[a] = 0 leaves the axis alone; a pad may exceed the side."""
    x = _ring_input(x, "ring_pad")
    B, C, T, H, W = geom(x)
    p = _per_axis(pad, x, "pad", "ring_pad")
    big = (T + 2 * p[0], H + 2 * p[1], W + 2 * p[2])
    out = x.new_empty((B, C) + (big if x.dim() == 5 else big[1:]))
    call("hpvg_ring_pad_f32", ptr(x), B * C, T, H, W, (ctypes.c_int * 3)(*p), ptr(out), stream())
    return out


def ring_crop(y, pad):
    """The inverse geometry of ring_pad: pad[a] voxels dropped from both ends of every spatial axis (hpvg_box_copy_f32)."""
    y = _ring_input(y, "ring_crop")
    B, C, T, H, W = geom(y)
    p = _per_axis(pad, y, "pad", "ring_crop")
    small = (T - 2 * p[0], H - 2 * p[1], W - 2 * p[2])
    if min(small) < 1:
        raise RuntimeError("ring_crop of %r leaves nothing of %s" % (p, tuple(y.shape)))
    out = y.new_empty((B, C) + (small if y.dim() == 5 else small[1:]))
    call("hpvg_box_copy_f32", ptr(y), ptr(out), B * C, T, H, W, *small, -p[0], -p[1], -p[2], stream())
    return out


def upsample_ring(x, size, wrap):
    """Linear resize of [B, C, (T,) H, W] to `size` whose axes flagged in `wrap` (one 0 / 1 per spatial axis) are rings: source
    coordinate o S / O, the last sample interpolating towards the first; the other axes as UpsampleAC
    (hpvg_upsample_linear_ring_f32)."""
    x = _ring_input(x, "upsample_ring")
    B, C, Ti, Hi, Wi = geom(x)
    size = tuple(int(s) for s in size)
    if len(size) != x.dim() - 2:
        raise ValueError("upsample_ring: size %r does not fit %s" % (size, tuple(x.shape)))
    w = _per_axis(wrap, x, "wrap", "upsample_ring")
    To, Ho, Wo = size if x.dim() == 5 else (1,) + size
    y = torch.empty((B, C) + size, dtype=torch.float32, device=x.device)
    call("hpvg_upsample_linear_ring_f32", ptr(x), B * C, Ti, Hi, Wi, ptr(y), To, Ho, Wo, (ctypes.c_int * 3)(*w), stream())
    return y


# ------------------------------------------------------------------------------------------ N(0,1) noise (Philox kernel)
class _RngState:
    """Counter-based noise stream of one device: (seed, iteration counter ON THE DEVICE, call index inside the iteration).
    The kernels read the iteration from device memory, so a hipGraph replay draws fresh noise although none of its launch
    arguments changes; the trainers bump it once per iteration (rng_next_iteration)."""

    def __init__(self, device):
        self.iter_dev = torch.zeros(1, dtype=torch.int32, device=device)
        self.call = 0


_rng_states = {}


def _rng(device):
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())   # "cuda" and "cuda:0" are one stream
    key = (device.type, device.index)
    st = _rng_states.get(key)
    if st is None:
        st = _rng_states[key] = _RngState(device)
    return st


def rng_next_iteration(device):
    """Start the noise stream of the next train iteration on `device` (one 1-thread kernel; captured with the iteration)."""
    st = _rng(torch.device(device) if not isinstance(device, torch.device) else device)
    counter_inc_(st.iter_dev)
    st.call = 0


def _seed():
    return torch.initial_seed() & 0xFFFFFFFFFFFFFFFF   # follows torch.manual_seed


def _philox_call(name, device, *args):
    """Launch a kernel whose arguments end in the Philox triple (seed, call index, iteration pointer) and the stream: the next
    draw of `device`'s noise stream."""
    st = _rng(device)
    call(name, *args, _seed(), st.call & 0xFFFFFFFF, ptr(st.iter_dev), stream())
    st.call += 1


def normal_(out):
    """out <- N(0, 1) (utils/images.py:49, networks_3d.py:32) with the Philox kernel of libhpvg; returns out."""
    _philox_call("hpvg_normal_f32", out.device, ptr(out), out.numel())
    return out


def uniform_(out):
    """out <- U[0, 1) from the library's Philox stream (reparameterize_bern's eps, networks_3d.py:40)."""
    _philox_call("hpvg_uniform_f32", out.device, ptr(out), out.numel())
    return out


# ------------------------------------------------------------------------------------------ variant models (the _nb family)
def _bcs(x):
    B, C = x.shape[0], x.shape[1]
    S = 1
    for d in x.shape[2:]:
        S *= int(d)
    return B, C, S


class Gate(Function):
    """(bern * f, bern) with bern = sigmoid(logit) broadcast over channels (Encode3DVAE_nb: networks_3d.py:131-133)."""

    @staticmethod
    def forward(ctx, f, logit):
        f, logit = _c(f), _c(logit)
        B, C, S = _bcs(f)
        out = torch.empty_like(f)
        bern = torch.empty_like(logit)
        call("hpvg_gate_fwd_f32", ptr(f), ptr(logit), ptr(out), ptr(bern), B, C, S, stream())
        ctx.save_for_backward(f, bern)
        return out, bern

    @staticmethod
    @once_differentiable
    def backward(ctx, dout, dbern):
        f, bern = ctx.saved_tensors
        B, C, S = _bcs(f)
        dout = _c(dout) if dout is not None else None
        dbern = _c(dbern) if dbern is not None else None
        df = torch.empty_like(f) if (ctx.needs_input_grad[0] and dout is not None) else None
        dlogit = torch.empty_like(bern) if ctx.needs_input_grad[1] else None
        call("hpvg_gate_bwd_f32", ptr(dout), ptr(f), ptr(bern), ptr(dbern), ptr(df), ptr(dlogit), B, C, S, stream())
        return df, dlogit


class GlobalAvgPool(Function):
    """nn.AdaptiveAvgPool3d(1) / AdaptiveAvgPool2d(1): [B, C, ...] -> [B, C, 1, (1,) 1] (networks_3d.py:121-128)."""

    @staticmethod
    def forward(ctx, x):
        x = _c(x)
        B, C, S = _bcs(x)
        out = torch.empty((B, C) + (1,) * (x.dim() - 2), dtype=torch.float32, device=x.device)
        call("hpvg_rowsum_f32", ptr(x), None, ptr(out), float(1.0 / S), B, C, S, stream())
        ctx.shape = x.shape
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        g = _c(g)
        B, C, S = _bcs(torch.empty(ctx.shape, device="meta"))
        dx = torch.empty(ctx.shape, dtype=torch.float32, device=g.device)
        call("hpvg_outer_f32", ptr(g), None, ptr(dx), float(1.0 / S), B, C, S, stream())
        return dx


class CodeTimesMap(Function):
    """z[b,c,s] = code[b,c] * map[b,s]: z_vae_norm [B,C,1,1,1] x z_vae_bern [B,1,T,H,W] (networks_3d.py:456)."""

    @staticmethod
    def forward(ctx, code, zmap):
        code, zmap = _c(code), _c(zmap)
        B, C = code.shape[0], code.shape[1]
        S = zmap.numel() // B
        if code.numel() != B * C or zmap.shape[1] != 1:
            raise RuntimeError("CodeTimesMap: expected a [B,C,1,..] code and a [B,1,...] map, got %s, %s" % (tuple(code.shape), tuple(zmap.shape)))
        out = torch.empty((B, C) + tuple(zmap.shape[2:]), dtype=torch.float32, device=code.device)
        call("hpvg_outer_f32", ptr(code), ptr(zmap), ptr(out), 1.0, B, C, S, stream())
        ctx.save_for_backward(code, zmap)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dz):
        code, zmap = ctx.saved_tensors
        dz = _c(dz)
        B, C = code.shape[0], code.shape[1]
        S = zmap.numel() // B
        dcode = dmap = None
        if ctx.needs_input_grad[0]:
            dcode = torch.empty_like(code)
            call("hpvg_rowsum_f32", ptr(dz), ptr(zmap), ptr(dcode), 1.0, B, C, S, stream())
        if ctx.needs_input_grad[1]:
            dmap = torch.empty_like(zmap)
            call("hpvg_colsum_f32", ptr(dz), ptr(code), ptr(dmap), B, C, S, stream())
        return dcode, dmap


class ReparamBern(Function):
    """log(x + 1e-20) - log(-log(eps + 1e-20) + 1e-20), eps ~ U(0,1) (reparameterize_bern, networks_3d.py:38-42)."""

    @staticmethod
    def forward(ctx, x, eps):
        x, eps = _c(x), _c(eps)
        z = torch.empty_like(x)
        call("hpvg_reparam_bern_fwd_f32", ptr(x), ptr(eps), ptr(z), x.numel(), stream())
        ctx.save_for_backward(x)
        return z

    @staticmethod
    @once_differentiable
    def backward(ctx, dz):
        (x,) = ctx.saved_tensors
        dx = torch.empty_like(x)
        call("hpvg_reparam_bern_bwd_f32", ptr(_c(dz)), ptr(x), ptr(dx), x.numel(), stream())
        return dx, None


class KLBern(Function):
    """mean(x (log(x+1e-20) - log .5) + (1-x)(log(1-x+1e-20) - log .5))  (kl_bern_criterion, modules/losses.py:12-14)."""

    @staticmethod
    def forward(ctx, x):
        x = _c(x)
        out = _scalar_out(x.device)
        call("hpvg_kl_bern_fwd_f32", ptr(x), ptr(out), *_reduce_ws(x.device), x.numel(), stream())
        ctx.save_for_backward(x)
        return out.view(())

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        dx = torch.empty_like(x)
        call("hpvg_kl_bern_bwd_f32", ptr(_c(g).view(1)), ptr(x), ptr(dx), x.numel(), stream())
        return dx


class UpsampleACNoise(Function):
    """(up, up + amp * N(0,1)) with the level noise generated inside the resize kernel (no noise tensor in memory);
    samples below `first_noisy` get no noise (the reconstruction half of a merged generator pass).  Same backward as
    UpsampleAC (the noise carries no gradient)."""

    @staticmethod
    def forward(ctx, x, size, amp, first_noisy):
        x = _c(x)
        y, dims = _resize_out(ctx, x, size)
        yn = torch.empty_like(y)
        _philox_call("hpvg_upsample_linear_ac_noise_f32", x.device, ptr(x), ptr(y), ptr(yn), float(amp), dims[0], x.shape[1],
                     int(first_noisy), *dims[1:])
        return y, yn

    backward = UpsampleAC.backward


class Reparam(Function):
    """z = eps * exp(0.5*logvar) + mu (networks_3d.py:29-33, training branch)."""

    @staticmethod
    def forward(ctx, mu, logvar, eps):
        mu, logvar, eps = _c(mu), _c(logvar), _c(eps)
        z = torch.empty_like(mu)
        call("hpvg_reparam_fwd_f32", ptr(mu), ptr(logvar), ptr(eps), ptr(z), mu.numel(), stream())
        ctx.save_for_backward(logvar, eps)
        return z

    @staticmethod
    @once_differentiable
    def backward(ctx, dz):
        logvar, eps = ctx.saved_tensors
        dz = _c(dz)
        dlv = torch.empty_like(dz)
        call("hpvg_reparam_bwd_f32", ptr(dz), ptr(logvar), ptr(eps), ptr(dlv), dz.numel(), stream())
        return dz, dlv, None


# ------------------------------------------------------------------------------------------ losses
class KL(Function):
    """mean(-0.5*(1 + logvar - mu^2 - exp(logvar)))  (modules/losses.py:7-9)."""

    @staticmethod
    def forward(ctx, mu, logvar):
        mu, logvar = _c(mu), _c(logvar)
        out = _scalar_out(mu.device)
        call("hpvg_kl_fwd_f32", ptr(mu), ptr(logvar), ptr(out), *_reduce_ws(mu.device), mu.numel(), stream())
        ctx.save_for_backward(mu, logvar)
        return out.view(())

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        mu, logvar = ctx.saved_tensors
        g = _c(g).view(1)
        dmu = torch.empty_like(mu)
        dlv = torch.empty_like(mu)
        call("hpvg_kl_bwd_f32", ptr(g), ptr(mu), ptr(logvar), ptr(dmu), ptr(dlv), mu.numel(), stream())
        return dmu, dlv


class MSE(Function):
    """mean((a-b)^2)  (nn.MSELoss: train_video.py:355)."""

    @staticmethod
    def forward(ctx, a, b):
        a, b = _c(a), _c(b)
        if a.shape != b.shape:
            raise RuntimeError("mse: shape mismatch %s vs %s" % (tuple(a.shape), tuple(b.shape)))
        out = _scalar_out(a.device)
        call("hpvg_mse_fwd_f32", ptr(a), ptr(b), ptr(out), *_reduce_ws(a.device), a.numel(), stream())
        ctx.save_for_backward(a, b)
        return out.view(())

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        g = _c(g).view(1)
        da = db = None
        if ctx.needs_input_grad[0]:
            da = torch.empty_like(a)
            call("hpvg_mse_bwd_f32", ptr(g), ptr(a), ptr(b), ptr(da), a.numel(), stream())
        if ctx.needs_input_grad[1]:
            db = torch.empty_like(a)
            call("hpvg_mse_bwd_f32", ptr(g), ptr(b), ptr(a), ptr(db), a.numel(), stream())
        return da, db


class MeanScaled(Function):
    """sign * mean(x): the WGAN critic terms (train_video.py:170,178,194)."""

    @staticmethod
    def forward(ctx, x, sign):
        x = _c(x)
        out = _scalar_out(x.device)
        call("hpvg_sum_scaled_f32", ptr(x), ptr(out), sign / x.numel(), *_reduce_ws(x.device), x.numel(), stream())
        ctx.shape = x.shape
        ctx.coef = sign / x.numel()
        return out.view(())

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        g = _c(g).view(1)
        dx = torch.empty(ctx.shape, dtype=torch.float32, device=g.device)
        call("hpvg_fill_scaled_f32", ptr(g), float(ctx.coef), ptr(dx), dx.numel(), stream())
        return dx, None


class GradPenalty(Function):
    """lambda * mean_{b,voxel} (||g[b,:,voxel]||_2 - 1)^2   (modules/utils.py:18; norm over dim=1)."""

    @staticmethod
    def forward(ctx, g, lam):
        g = _c(g)
        B, C, T, H, W = geom(g)
        out = _scalar_out(g.device)
        call("hpvg_gp_fwd_f32", ptr(g), ptr(out), float(lam), *_reduce_ws(g.device), B, C, T * H * W, stream())
        ctx.save_for_backward(g)
        ctx.lam = lam
        return out.view(())

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        (g,) = ctx.saved_tensors
        gout = _c(gout).view(1)
        B, C, T, H, W = geom(g)
        dg = torch.empty_like(g)
        call("hpvg_gp_bwd_f32", ptr(gout), ptr(g), ptr(dg), float(ctx.lam), B, C, T * H * W, stream())
        return dg, None


_pinned_ring = []


def host_floats_to_device(values, device):
    """A few host floats -> a device tensor WITHOUT stalling the host: a plain `.to(device)` from pageable memory is a
    synchronous copy on the compute stream, i.e. the host waits for every kernel queued so far (the whole iteration up to
    the gradient penalty's alpha) and then has to re-fill the queue.  Staged through a small ring of pinned buffers."""
    vals = [float(v) for v in values]
    if device.type != "cuda":
        return torch.tensor(vals, dtype=torch.float32, device=device)
    if not _pinned_ring:
        _pinned_ring.extend([0, [torch.empty(16, dtype=torch.float32).pin_memory() for _ in range(16)]])
    slot = _pinned_ring[1][_pinned_ring[0] % 16]
    _pinned_ring[0] += 1
    for i, v in enumerate(vals):
        slot[i] = v
    return slot[:len(vals)].to(device, non_blocking=True)


def lerp(a, b, alpha):
    """alpha*a + (1-alpha)*b with a device scalar alpha (no autograd: the result becomes a leaf, modules/utils.py:9-10)."""
    a, b = _c(a.detach()), _c(b.detach())
    out = torch.empty_like(a)
    call("hpvg_lerp_f32", ptr(a), ptr(b), ptr(alpha), ptr(out), a.numel(), stream())
    return out


# ------------------------------------------------------------------------------------------ optimizer primitives
def sqsum(flat):
    out = _scalar_out(flat.device)
    call("hpvg_sqsum_f32", ptr(flat), ptr(out), *_reduce_ws(flat.device), flat.numel(), stream())
    return out


def clip_scale_(flat_grad, sq, max_norm, coef_out=None):
    call("hpvg_clip_scale_f32", ptr(flat_grad), flat_grad.numel(), ptr(sq), float(max_norm), ptr(coef_out),
         stream())


def adam_step_(p, g, m, v, lr, beta1, beta2, eps, step, step_dev=None):
    weights_changed()
    call("hpvg_adam_step_f32", ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), float(lr), float(beta1), float(beta2),
         float(eps), int(step), ptr(step_dev), stream())


def counter_inc_(counter):
    call("hpvg_counter_inc_i32", ptr(counter), stream())


def state_digest_(t, salt, acc):
    """acc[0] (int64 device word) += the digest of t's 32-bit words keyed from position `salt` (hpvg_state_digest_u32);
    returns the number of words.  4-byte and 8-byte dtypes; an 8-byte element counts as two words, low word first."""
    if t.element_size() not in (4, 8):
        raise RuntimeError("state_digest: 4-byte and 8-byte dtypes only, got %s" % t.dtype)
    t = _c(t.detach())
    n = t.numel() * (t.element_size() // 4)
    call("hpvg_state_digest_u32", ptr(t) if n else None, n, int(salt) & 0xFFFFFFFFFFFFFFFF, ptr(acc), stream())
    return n


def state_digest(tensors):
    """64-bit digest (a python int) of the device tensors' bits, in order: each tensor's salt is the number of words digested
    before it, so the result is that of one call over their concatenation.  Reading the result synchronises the stream."""
    tensors = list(tensors)
    if not tensors:
        return 0
    acc = torch.zeros(1, dtype=torch.int64, device=tensors[0].device)
    salt = 0
    for t in tensors:
        salt += state_digest_(t, salt, acc)
    return int(acc.item()) & 0xFFFFFFFFFFFFFFFF


# ------------------------------------------------------------------------------------------ the programs' outputs
def video_to_u8(x):
    """fp32 [B][C][T][H][W] (or an image batch [B][C][H][W]) -> uint8 [B][T][H][W][C] (images: [B][H][W][C]) with write_video's
    np.uint8((x + 1) * 127.5) (utils/saver.py:8-19): truncation, clamped to [0, 255], NaN -> 0 (hpvg_video_to_u8_f32)."""
    x = _c(x)
    if x.dtype != torch.float32:
        raise RuntimeError("video_to_u8: fp32 input expected, got %s" % x.dtype)
    if x.dim() == 4:
        B, C, H, W = x.shape
        T = 1
        out = torch.empty(B, H, W, C, dtype=torch.uint8, device=x.device)
    elif x.dim() == 5:
        B, C, T, H, W = x.shape
        out = torch.empty(B, T, H, W, C, dtype=torch.uint8, device=x.device)
    else:
        raise RuntimeError("video_to_u8: expected [B,C,T,H,W] or [B,C,H,W], got %s" % (tuple(x.shape),))
    if out.numel():
        call("hpvg_video_to_u8_f32", ptr(x), ptr(out), B, C, T, H, W, stream())
    return out


def _triple(v, name, op="patch_nn"):
    v = tuple(int(e) for e in v)
    if len(v) != 3:
        raise RuntimeError("%s: %s must have 3 entries (t, h, w), got %d" % (op, name, len(v)))
    return (ctypes.c_int * 3)(*v)


def patch_nn_counts(qshape, rshape, patch, qstride=(1, 1, 1), rstride=(1, 1, 1)):
    """(Nq, Nr, D) of a patch_nn call on volumes of (T, H, W) = qshape / rshape (hpvg_patchnn_counts; host only)."""
    out = (ctypes.c_int * 3)()
    call("hpvg_patchnn_counts", *(int(e) for e in qshape), *(int(e) for e in rshape), _triple(patch, "patch"),
         _triple(qstride, "qstride"), _triple(rstride, "rstride"), out)
    return out[0], out[1], out[2]


def _patch_volumes(op, pairs):
    """The uint8 [T,H,W,3] views of volumes or images (all of one rank, on one device), and whether they are images."""
    vols = []
    for name, t in pairs:
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() not in (3, 4) or t.shape[-1] != 3:
            raise RuntimeError("%s: %s must be uint8 [T,H,W,3] or [H,W,3], got %s %s"
                               % (op, name, getattr(t, "dtype", type(t)), tuple(getattr(t, "shape", ()))))
        if t.dim() != pairs[0][1].dim():
            raise RuntimeError("%s: %s and %s must both be volumes or both be images" % (op, pairs[0][0], name))
        if t.device != pairs[0][1].device:
            raise RuntimeError("%s: %s on %s, %s on %s" % (op, pairs[0][0], pairs[0][1].device, name, t.device))
        vols.append(_c(t if t.dim() == 4 else t[None]))
    return vols, pairs[0][1].dim() == 3


# what every patch op works out before its launch: the contiguous volumes (r is q for a single-volume op), whether they are
# images, the C triples, both (T, H, W), the counts of hpvg_patchnn_counts and both patch grids
_PatchArgs = collections.namedtuple("_PatchArgs", "q r image pa qs rs qg rg Nq Nr D grid rgrid")


def _patch_geom(op, q, r, image, patch, qstride, rstride, qname="qstride", rname="rstride"):
    """The _PatchArgs of volumes that are already [T,H,W,...]: triples refused by name, then hpvg_patchnn_counts, which refuses
    every other bad argument by name."""
    pa, qs, rs = _triple(patch, "patch", op), _triple(qstride, qname, op), _triple(rstride, rname, op)
    qg, rg = tuple(q.shape[:3]), tuple(r.shape[:3])
    counts = (ctypes.c_int * 3)()
    call("hpvg_patchnn_counts", *qg, *rg, pa, qs, rs, counts)
    grid = tuple((qg[a] - pa[a]) // qs[a] + 1 for a in range(3))
    rgrid = tuple((rg[a] - pa[a]) // rs[a] + 1 for a in range(3))
    return _PatchArgs(q, r, image, pa, qs, rs, qg, rg, counts[0], counts[1], counts[2], grid, rgrid)


def _patch_args(op, pairs, patch, *strides):
    """_patch_volumes, then _patch_geom: a (query, ref) op brings two pairs and two strides, a single-volume op one of each."""
    vols, image = _patch_volumes(op, pairs)
    if len(vols) == 1:
        return _patch_geom(op, vols[0], vols[0], image, patch, strides[0], strides[0], "stride", "stride")
    return _patch_geom(op, vols[0], vols[1], image, patch, *strides)


def _per_ref_patch(op, name, t, dtype, Nr, rgrid, image, device):
    """A tensor with one entry per patch of ref's grid (flat, or shaped as the grid), contiguous; its values are the caller's."""
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.device != device or \
            tuple(t.shape) not in ((Nr,), rgrid, rgrid[1:] if image else rgrid):
        raise RuntimeError("%s: %s must be %s [%d] or %s on %s, got %s %s on %s"
                           % (op, name, str(dtype)[6:], Nr, rgrid[1:] if image else rgrid, device, getattr(t, "dtype", type(t)),
                              tuple(getattr(t, "shape", ())), getattr(t, "device", None)))
    return _c(t)


def _ref_weight(op, w, a):
    w = _per_ref_patch(op, "ref_weight", w, torch.float32, a.Nr, a.rgrid, a.image, a.r.device)
    if not bool((torch.isfinite(w) & (w > 0)).all()):   # one device reduction
        raise RuntimeError("%s: every ref_weight must be finite and > 0" % op)
    return w


def _ungrid(image, *outs):
    """Outputs shaped as [gT,gH,gW,...] patch grids, without the leading 1 for images; one output comes back bare."""
    outs = tuple(o[0] for o in outs) if image else outs
    return outs[0] if len(outs) == 1 else outs


def patch_nn(query_u8, ref_u8, patch, qstride=(1, 1, 1), rstride=(1, 1, 1)):
    """Exact patch nearest neighbours (hpvg_patchnn_u8, i8 matrix cores): query / ref are uint8 device tensors [T,H,W,3] or
    [H,W,3]; for every patch of the query's strided grid, d2 = the smallest squared distance to a patch of ref's grid and nn =
    the smallest index (raster order of ref's grid) that attains it.  Both int32, shaped as the query's patch grid."""
    a = _patch_args("patch_nn", (("query", query_u8), ("ref", ref_u8)), patch, qstride, rstride)
    ws = _scratch(call("hpvg_patchnn_ws_bytes", *a.qg, *a.rg, a.pa, a.qs, a.rs), a.q.device)
    d2 = torch.empty(a.grid, dtype=torch.int32, device=a.q.device)
    nn = torch.empty(a.grid, dtype=torch.int32, device=a.q.device)
    call("hpvg_patchnn_u8", ptr(a.q), *a.qg, ptr(a.r), *a.rg, a.pa, a.qs, a.rs, ptr(d2), ptr(nn), *ws, stream())
    return _ungrid(a.image, d2, nn)


def patch_nn_weighted(query_u8, ref_u8, ref_weight, patch, qstride=(1, 1, 1), rstride=(1, 1, 1)):
    """patch_nn with a weight per reference patch (hpvg_patchnn_weighted_u8, i8 matrix cores; GPNN's completeness
    normalisation): score = min_j float32(d2_ij) * ref_weight[j], the exact int32 distance converted and multiplied once in
    fp32, and nn = the smallest j that attains it.  ref_weight: float32 device tensor of Nr entries (flat, or shaped as ref's
    patch grid), every one finite and > 0.  Returns (score float32, nn int32), shaped as the query's patch grid."""
    a = _patch_args("patch_nn_weighted", (("query", query_u8), ("ref", ref_u8)), patch, qstride, rstride)
    w = _ref_weight("patch_nn_weighted", ref_weight, a)
    ws = _scratch(call("hpvg_patchnn_ws_bytes", *a.qg, *a.rg, a.pa, a.qs, a.rs), a.q.device)
    score = torch.empty(a.grid, dtype=torch.float32, device=a.q.device)
    nn = torch.empty(a.grid, dtype=torch.int32, device=a.q.device)
    call("hpvg_patchnn_weighted_u8", ptr(a.q), *a.qg, ptr(a.r), *a.rg, a.pa, a.qs, a.rs, ptr(w), ptr(score), ptr(nn), *ws, stream())
    return _ungrid(a.image, score, nn)


def _wrap_flags(wrap, name, op):
    """Ring flags (wt, wh, ww), each 0 / 1 (or a bool), as a C int[3]; None stays None (a null pointer: no rings)."""
    if wrap is None:
        return None
    w = tuple(wrap)
    if len(w) != 3 or any(e not in (0, 1) for e in w):
        raise RuntimeError("%s: %s must be three flags (t, h, w), each 0 or 1, got %r" % (op, name, wrap))
    return (ctypes.c_int * 3)(*(int(e) for e in w))


def patch_match(query_u8, ref_u8, patch, iters, seed=0, ref_weight=None, nn_init=None, qwrap=None, rwrap=None):
    """Deterministic PatchMatch (hpvg_patchmatch_u8): an approximate nearest-neighbour field between the dense patch grids of two
    uint8 device tensors [T,H,W,3] or [H,W,3], at a cost linear in the number of patches.  The rule - hash start or nn_init,
    `iters` Jacobi iterations of propagation and a shrinking random search, keys (d2, j) or (float32(d2) * ref_weight[j], j) -
    is written out in include/hpvg.h; a seed gives the same field on every run.  ref_weight: as for patch_nn_weighted.
    nn_init: int32 device tensor with the query grid's element count (entries are clamped into the key grid).  Returns
    (d2 int32, nn int32), or (score float32, nn int32) with weights, shaped as the query's patch grid.
    qwrap / rwrap (hpvg_patchmatch_wrap_u8): flags (t, h, w) saying which axes of the query's / ref's PATCH GRID are rings; the
    volume on a ring side arrives circularly padded by the caller, so its dense grid is the periodic one.  Both None: the plain
    entry point, exactly as before."""
    (q, r), image = _patch_volumes("patch_match", (("query", query_u8), ("ref", ref_u8)))
    qw, rw = _wrap_flags(qwrap, "qwrap", "patch_match"), _wrap_flags(rwrap, "rwrap", "patch_match")
    a = _patch_geom("patch_match", q, r, image, patch, (1, 1, 1), (1, 1, 1))
    w = _ref_weight("patch_match", ref_weight, a) if ref_weight is not None else None
    if nn_init is not None:
        if not isinstance(nn_init, torch.Tensor) or nn_init.dtype != torch.int32 or nn_init.numel() != a.Nq or nn_init.device != q.device:
            raise RuntimeError("patch_match: nn_init must be int32 with %d entries on %s, got %s %s on %s"
                               % (a.Nq, q.device, getattr(nn_init, "dtype", type(nn_init)), tuple(getattr(nn_init, "shape", ())),
                                  getattr(nn_init, "device", None)))
        nn_init = _c(nn_init)
    nbytes = call("hpvg_patchmatch_ws_bytes", *a.qg, *a.rg, a.pa)
    if nbytes == 0 or not 0 <= int(iters) <= 1024:
        raise RuntimeError("patch_match: refused (a patch grid side >= 65536, or iters %r outside [0, 1024])" % (iters,))
    ws = _scratch(nbytes, q.device)
    d2 = torch.empty(a.grid, dtype=torch.int32, device=q.device)
    nn = torch.empty(a.grid, dtype=torch.int32, device=q.device)
    score = torch.empty(a.grid, dtype=torch.float32, device=q.device) if w is not None else None
    if qw is None and rw is None:
        call("hpvg_patchmatch_u8", ptr(q), *a.qg, ptr(r), *a.rg, a.pa, ptr(w), ptr(nn_init), int(iters), int(seed), ptr(d2), ptr(nn),
             ptr(score), *ws, stream())
    else:
        call("hpvg_patchmatch_wrap_u8", ptr(q), *a.qg, ptr(r), *a.rg, a.pa, qw, rw, ptr(w), ptr(nn_init), int(iters), int(seed), ptr(d2),
             ptr(nn), ptr(score), *ws, stream())
    return _ungrid(image, score if w is not None else d2, nn)


def _patch_sel(sel, name, N, device):
    """A subset search's list as launch arguments (pointer, count, the tensor kept alive); None is the whole grid.  Checked on
    the device with one reduction: int32, 1-D, non-empty, strictly ascending, within [0, N)."""
    if sel is None:
        return None, 0, None
    if not isinstance(sel, torch.Tensor) or sel.dtype != torch.int32 or sel.dim() != 1 or sel.numel() < 1 or sel.device != device:
        raise RuntimeError("patch_nn_subset: %s must be a non-empty 1-D int32 tensor on %s, got %s %s on %s"
                           % (name, device, getattr(sel, "dtype", type(sel)), tuple(getattr(sel, "shape", ())),
                              getattr(sel, "device", None)))
    sel = _c(sel)
    if not bool((sel[0] >= 0) & (sel[-1] < N) & (sel[1:] > sel[:-1]).all()):
        raise RuntimeError("patch_nn_subset: %s must be strictly ascending with every entry in [0, %d)" % (name, N))
    return ptr(sel), sel.numel(), sel


def patch_nn_subset(query_u8, ref_u8, patch, qsel=None, rsel=None, qstride=(1, 1, 1), rstride=(1, 1, 1)):
    """patch_nn over selected patches of both grids (hpvg_patchnn_subset_u8, i8 matrix cores; the search of patch inpainting):
    qsel / rsel are 1-D int32 device tensors of flat grid indices (raster order), strictly ascending; None is the whole grid.
    Only the selected patches are packed and compared.  Returns (d2, nn), int32, shaped as the query's patch grid: for a
    selected query patch the smallest squared distance to a selected patch of ref and the smallest index IN REF'S GRID that
    attains it; -1, -1 for every other patch (patch_vote skips those)."""
    a = _patch_args("patch_nn_subset", (("query", query_u8), ("ref", ref_u8)), patch, qstride, rstride)
    qp, nq, qkeep = _patch_sel(qsel, "qsel", a.Nq, a.q.device)
    rp, nr, rkeep = _patch_sel(rsel, "rsel", a.Nr, a.q.device)
    # the workspace query has no list pointers to tell a null list by: there a negative count stands for one (the search itself
    # takes the null pointer and ignores the count)
    nbytes = call("hpvg_patchnn_subset_ws_bytes", *a.qg, *a.rg, a.pa, a.qs, a.rs, nq if qsel is not None else -1,
                  nr if rsel is not None else -1)
    ws = _scratch(nbytes, a.q.device)
    d2 = torch.empty(a.grid, dtype=torch.int32, device=a.q.device)
    nn = torch.empty(a.grid, dtype=torch.int32, device=a.q.device)
    call("hpvg_patchnn_subset_u8", ptr(a.q), *a.qg, ptr(a.r), *a.rg, a.pa, a.qs, a.rs, qp, nq, rp, nr, ptr(d2), ptr(nn), *ws, stream())
    return _ungrid(a.image, d2, nn)


def patch_mask_count(mask_u8, patch, stride=(1, 1, 1)):
    """For every patch of the strided grid of a uint8 device mask [T,H,W] (or [H,W]; nonzero = hole) the number of hole voxels
    under it (hpvg_patch_mask_count_u8): int32, shaped as the patch grid, 0 for a patch that avoids the hole."""
    m = mask_u8
    if not isinstance(m, torch.Tensor) or m.dtype != torch.uint8 or m.dim() not in (2, 3):
        raise RuntimeError("patch_mask_count: mask must be uint8 [T,H,W] or [H,W], got %s %s"
                           % (getattr(m, "dtype", type(m)), tuple(getattr(m, "shape", ()))))
    image = m.dim() == 2
    m = _c(m[None] if image else m)
    a = _patch_geom("patch_mask_count", m, m, image, patch, stride, stride, "stride", "stride")
    count = torch.empty(a.grid, dtype=torch.int32, device=m.device)
    call("hpvg_patch_mask_count_u8", ptr(m), *a.qg, a.pa, a.qs, ptr(count), stream())
    return _ungrid(image, count)


PATCH_KNN_MAX_K = 8   # hpvg_patchknn_self_u8 keeps at most this many distances per patch


def patch_knn_self(vol_u8, patch, k, stride=(1, 1, 1)):
    """The k smallest exact squared distances from every patch of a volume to the OTHER patches of the same strided grid
    (hpvg_patchknn_self_u8, i8 matrix cores, one pass): vol is a uint8 device tensor [T,H,W,3] or [H,W,3], 1 <= k <= 8 < the
    patch count.  Returns int32 [gT,gH,gW,k] ([gH,gW,k] for an image), ascending along the last axis and with multiplicity: a
    patch is excluded from its own list by index, so an exact duplicate elsewhere contributes a 0.  [..., k-1] is the radius
    of improved precision / recall."""
    a = _patch_args("patch_knn_self", (("vol", vol_u8),), patch, stride)
    if isinstance(k, bool) or not isinstance(k, int) or k < 1 or k > PATCH_KNN_MAX_K:
        raise RuntimeError("patch_knn_self: k must be an int in [1, %d], got %r" % (PATCH_KNN_MAX_K, k))
    if a.Nq <= k:
        raise RuntimeError("patch_knn_self: %d patches cannot have %d neighbours each (the patch count must exceed k)" % (a.Nq, k))
    ws = _scratch(call("hpvg_patchknn_self_ws_bytes", *a.qg, a.pa, a.qs, k), a.q.device)
    kth = torch.empty(a.grid + (k,), dtype=torch.int32, device=a.q.device)
    call("hpvg_patchknn_self_u8", ptr(a.q), *a.qg, a.pa, a.qs, k, ptr(kth), *ws, stream())
    return _ungrid(a.image, kth)


def patch_ball_count(query_u8, ref_u8, ref_radius, patch, qstride=(1, 1, 1), rstride=(1, 1, 1)):
    """For every patch of the query's strided grid the number of patches j of ref's grid with d2(q_i, r_j) <= ref_radius[j]
    (hpvg_patch_ball_count_u8, i8 matrix cores; d2 the exact squared distance of patch_nn).  ref_radius: int32 device tensor of
    Nr entries (flat, or shaped as ref's patch grid), every one >= 0.  Returns int32 shaped as the query's patch grid; > 0 is
    "inside some ball" (precision / recall), the sum is the numerator of density."""
    a = _patch_args("patch_ball_count", (("query", query_u8), ("ref", ref_u8)), patch, qstride, rstride)
    rad = _per_ref_patch("patch_ball_count", "ref_radius", ref_radius, torch.int32, a.Nr, a.rgrid, a.image, a.r.device)
    if not bool((rad >= 0).all()):   # one device reduction
        raise RuntimeError("patch_ball_count: every ref_radius must be >= 0")
    ws = _scratch(call("hpvg_patch_ball_count_ws_bytes", *a.qg, *a.rg, a.pa, a.qs, a.rs), a.q.device)
    count = torch.empty(a.grid, dtype=torch.int32, device=a.q.device)
    call("hpvg_patch_ball_count_u8", ptr(a.q), *a.qg, ptr(a.r), *a.rg, a.pa, a.qs, a.rs, ptr(rad), ptr(count), *ws, stream())
    return _ungrid(a.image, count)


def nnf_chunks(nn, ref_grid, qstride=(1, 1, 1), rstride=(1, 1, 1), d2=None, max_d2=None):
    """The copied regions of a nearest-neighbour field (hpvg_nnf_chunks_i32, a union-find over the patch grid): nn is an int32
    device tensor shaped as a query patch grid [gT,gH,gW] (or [gH,gW], as patch_nn returns it for images: gT = 1) of indices
    into the key patch grid ref_grid = (kT, kH, kW).  A patch is kept iff its index is in range and, with d2 (int32, shaped as
    nn) and max_d2 given, 0 <= d2 <= max_d2; two 6-neighbours are joined iff both are kept and their displacements
    key coordinate * rstride - grid coordinate * qstride are equal.  Returns (labels, sizes, stats): labels int32 shaped as nn
    (the smallest flat index of the patch's chunk, -1 where not kept), sizes int32 shaped as nn (the chunk's size at its label,
    0 elsewhere) and stats int64 [6] = kept, in_place, coherent_pairs, chunks, largest, sum of size^2.  Exact."""
    if not isinstance(nn, torch.Tensor) or nn.dtype != torch.int32 or nn.dim() not in (2, 3) or nn.numel() < 1:
        raise RuntimeError("nnf_chunks: nn must be a non-empty int32 patch grid [gT,gH,gW] or [gH,gW], got %s %s"
                           % (getattr(nn, "dtype", type(nn)), tuple(getattr(nn, "shape", ()))))
    if not nn.is_cuda:
        raise RuntimeError("nnf_chunks: nn is on %s; this op runs only on an MI355X device (no CPU fallback)" % nn.device)
    if (d2 is None) != (max_d2 is None):
        raise RuntimeError("nnf_chunks: d2 and max_d2 go together, got d2 %s and max_d2 %s"
                           % ("None" if d2 is None else "given", max_d2))
    if d2 is not None:
        if not isinstance(d2, torch.Tensor) or d2.dtype != torch.int32 or d2.shape != nn.shape or d2.device != nn.device:
            raise RuntimeError("nnf_chunks: d2 must be int32 %s on %s like nn, got %s %s on %s"
                               % (tuple(nn.shape), nn.device, getattr(d2, "dtype", type(d2)), tuple(getattr(d2, "shape", ())),
                                  getattr(d2, "device", None)))
        if int(max_d2) < 0 or int(max_d2) >= 2 ** 31:
            raise RuntimeError("nnf_chunks: max_d2 must be in [0, 2^31), got %s" % (max_d2,))
        d2 = _c(d2)
    image = nn.dim() == 2
    n = _c(nn[None] if image else nn)
    qg = _triple(n.shape, "nn's grid", "nnf_chunks")
    rg, qs, rs = _triple(ref_grid, "ref_grid", "nnf_chunks"), _triple(qstride, "qstride", "nnf_chunks"), \
        _triple(rstride, "rstride", "nnf_chunks")
    if min(rg) < 1 or rg[0] * rg[1] * rg[2] >= 2 ** 31:
        raise RuntimeError("nnf_chunks: ref_grid %s must have entries >= 1 and fewer than 2^31 patches" % (tuple(rg),))
    if min(qs) < 1 or min(rs) < 1:
        raise RuntimeError("nnf_chunks: strides must be >= 1, got qstride %s rstride %s" % (tuple(qs), tuple(rs)))
    labels = torch.empty_like(n)
    sizes = torch.empty_like(n)
    stats = torch.empty(6, dtype=torch.int64, device=n.device)
    call("hpvg_nnf_chunks_i32", ptr(n), ptr(d2), int(max_d2) if d2 is not None else 0, qg, rg, qs, rs, ptr(labels), ptr(sizes),
         ptr(stats), stream())
    if image:
        labels, sizes = labels[0], sizes[0]
    return labels, sizes, stats


def patch_vote_counts(out_shape, values_shape, patch, qstride=(1, 1, 1), rstride=(1, 1, 1)):
    """(Nq, Nr, uncovered) of a patch_vote call: the patches of the output's grid, those of the values volume's grid, and the
    output voxels no patch of the output's grid covers, which take the fallback (hpvg_patch_vote_counts; host only)."""
    out = (ctypes.c_long * 3)()
    call("hpvg_patch_vote_counts", *(int(e) for e in out_shape), *(int(e) for e in values_shape), _triple(patch, "patch", "patch_vote"),
         _triple(qstride, "qstride", "patch_vote"), _triple(rstride, "rstride", "patch_vote"), out)
    return out[0], out[1], out[2]


def patch_vote(values_u8, nn, patch, out_shape, fallback_u8, qstride=(1, 1, 1), rstride=(1, 1, 1), wrap=None):
    """Rebuild a volume from chosen patches (hpvg_patch_vote_u8; the fold of the patch nearest-neighbour generator): every
    output voxel is the mean, halves rounded up, of the bytes that the patches of the output's grid (qstride) covering it take
    from the patches nn[i] of values_u8's grid (rstride).  values_u8 / fallback_u8: uint8 device tensors [T,H,W,3] or [H,W,3];
    out_shape = fallback's (T, H, W) or (H, W); nn: int32 with one entry per patch of the output's grid.  Entries outside
    [0, Nr) are skipped, and a voxel with no vote takes fallback's byte.  Returns a new uint8 tensor shaped as fallback_u8.
    wrap (hpvg_patch_vote_wrap_u8): flags (t, h, w) saying which axes of the OUTPUT are rings; the output's grid is then the
    periodic one (a whole side of positions on a ring axis, patches continuing from the last slice into the first), dense
    (qstride must be (1, 1, 1)), and nn has one entry per patch of it.  None: the plain entry point, exactly as before."""
    (v, fb), image = _patch_volumes("patch_vote", (("values", values_u8), ("fallback", fallback_u8)))
    wr = _wrap_flags(wrap, "wrap", "patch_vote")
    oshape = tuple(int(e) for e in out_shape)
    if oshape != tuple(fallback_u8.shape[:-1]):
        raise RuntimeError("patch_vote: out_shape %s is not the fallback's %s" % (oshape, tuple(fallback_u8.shape[:-1])))
    pa, qs, rs = _triple(patch, "patch", "patch_vote"), _triple(qstride, "qstride", "patch_vote"), _triple(rstride, "rstride", "patch_vote")
    og, vg = tuple(fb.shape[:3]), tuple(v.shape[:3])
    Nq = patch_vote_counts(og, vg, patch, qstride, rstride)[0]    # refuses bad arguments by name
    if wr is not None:
        if tuple(qs) != (1, 1, 1):
            raise RuntimeError("patch_vote: a ring's grid is dense: wrap needs qstride (1, 1, 1), got %s" % (tuple(qs),))
        Nq = 1
        for a in range(3):
            Nq *= og[a] if wr[a] else og[a] - pa[a] + 1
    if not isinstance(nn, torch.Tensor) or nn.dtype != torch.int32 or nn.numel() != Nq or nn.device != v.device:
        raise RuntimeError("patch_vote: nn must be int32 with %d entries on %s, got %s %s on %s"
                           % (Nq, v.device, getattr(nn, "dtype", type(nn)), tuple(getattr(nn, "shape", ())), getattr(nn, "device", None)))
    nn = _c(nn)
    out = torch.empty_like(fb)
    if wr is None:
        call("hpvg_patch_vote_u8", ptr(v), *vg, ptr(nn), *og, pa, qs, rs, ptr(fb), ptr(out), stream())
    else:
        call("hpvg_patch_vote_wrap_u8", ptr(v), *vg, ptr(nn), *og, pa, rs, wr, ptr(fb), ptr(out), stream())
    return out[0] if image else out


def volume_resize_check(src_size, out_size):
    """(Dmax, reads) of a volume_resize_u8 call from (T, H, W) = src_size to out_size: the largest denominator over the outputs
    and the largest number of source voxels one output reads (hpvg_volume_resize_check; host only).  Raises on a refusal."""
    out = (ctypes.c_long * 2)()
    call("hpvg_volume_resize_check", *_triple(src_size, "src_size", "volume_resize"), *_triple(out_size, "out_size", "volume_resize"), out)
    return out[0], out[1]


def volume_resize_u8(vol_u8, size):
    """The exact antialiased resize of a uint8 device volume [T,H,W,3] to (T, H, W) = size (hpvg_volume_resize_u8): per axis the
    integer weights max(0, R - |i (O - 1) - o (S - 1)|), R = max(O - 1, S - 1) - linear align-corners interpolation when
    upsizing, the triangle filter over everything an output voxel stands for when downsizing - and one rounding (halves up) of
    the separable weighted mean.  An image [H,W,3] is the volume with T = 1 and takes a size of 2 entries (or 3 with T = 1).
    An equal size returns a contiguous copy.  Returns a new uint8 tensor."""
    (src,), image = _patch_volumes("volume_resize_u8", (("the volume", vol_u8),))
    size = tuple(int(e) for e in size)
    if len(size) not in ((2, 3) if image else (3,)) or (image and len(size) == 3 and size[0] != 1):
        raise RuntimeError("volume_resize_u8: size must be (T, H, W)%s, got %s" % (" or (H, W) with T = 1" if image else "", size))
    if image and len(size) == 2:
        size = (1,) + size
    ptr(src)  # refuses a host tensor by name
    sg = tuple(src.shape[:3])
    volume_resize_check(sg, size)   # refuses bad sizes by name
    if sg == size:
        out = src.clone()
    else:
        out = torch.empty(size + (3,), dtype=torch.uint8, device=src.device)
        call("hpvg_volume_resize_u8", ptr(src), *sg, ptr(out), *size, stream())
    return out[0] if image else out


MASK_BLEND_MAX_RADIUS = 64   # hpvg_mask_blend_u8 takes radii in [0, 64]


def mask_blend(a_u8, b_u8, mask, radius):
    """The dilate-and-feather composite of two uint8 device volumes [T,H,W,3] (hpvg_mask_blend_u8): `a` inside the hole `mask`
    ([T,H,W], uint8 or bool, nonzero = hole), `b` farther than twice the radius from it, the exact integer blend
    (2 (c a + (n - c) b) + n) / (2 n) in between, c the dilated hole's voxels in the clipped box of radius = (rt, rh, rw) around
    the voxel and n the box's (include/hpvg.h).  Radius (0, 0, 0) is the hard composite.  Images [H,W,3] with a mask [H,W] are
    the volume with T = 1 and take a radius of 2 entries (or 3 with rt = 0).  Returns a new uint8 tensor shaped as `a`."""
    (a, b), image = _patch_volumes("mask_blend", (("a", a_u8), ("b", b_u8)))
    if a.shape != b.shape:
        raise RuntimeError("mask_blend: a %s and b %s must have one shape" % (tuple(a_u8.shape), tuple(b_u8.shape)))
    m = mask
    if not isinstance(m, torch.Tensor) or m.dtype not in (torch.uint8, torch.bool) or tuple(m.shape) != tuple(a_u8.shape[:-1]) or \
            m.device != a.device:
        raise RuntimeError("mask_blend: mask must be uint8 or bool %s on %s, got %s %s on %s"
                           % (tuple(a_u8.shape[:-1]), a.device, getattr(m, "dtype", type(m)), tuple(getattr(m, "shape", ())),
                              getattr(m, "device", None)))
    m = _c(m.to(torch.uint8))
    rad = tuple(int(e) for e in radius)
    if len(rad) not in ((2, 3) if image else (3,)) or (image and len(rad) == 3 and rad[0] != 0):
        raise RuntimeError("mask_blend: radius must be (rt, rh, rw)%s, got %s" % (" or (rh, rw): an image has rt = 0" if image else "", rad))
    if image and len(rad) == 2:
        rad = (0,) + rad
    if min(rad) < 0 or max(rad) > MASK_BLEND_MAX_RADIUS:
        raise RuntimeError("mask_blend: every radius must lie in [0, %d], got %s" % (MASK_BLEND_MAX_RADIUS, rad))
    ptr(a)  # refuses a host tensor by name
    T, H, W = (int(e) for e in a.shape[:3])
    rp = _triple(rad, "radius", "mask_blend")
    ws = _scratch(call("hpvg_mask_blend_ws_bytes", T, H, W, rp), a.device)
    out = torch.empty_like(a)
    call("hpvg_mask_blend_u8", ptr(a), ptr(b), ptr(m), T, H, W, rp, ptr(out), *ws, stream())
    return out[0] if image else out


# one hpvg_patchproj_hist_u8 launch fills at most this many bytes of histogram: the atomics' footprint stays within the 256 MB
# last-level cache, and the benchmarked case (512 directions at 3 x 7 x 7: 231 MB) is still one launch.  More directions go in
# chunks of whole 128-direction tiles (one direction at a time where a single histogram row passes the cap), each chunk packing
# the volume's patches again.
PATCH_PROJ_HIST_CAP_BYTES = 256 << 20


def patch_proj_bins(patch):
    """NB = 256 D + 1, the bins of one direction's projection histogram for this patch (hpvg_patchproj_bins; host only)."""
    nb = call("hpvg_patchproj_bins", _triple(patch, "patch", "patch_proj_hist"))
    if nb == 0:
        raise RuntimeError("patch_proj_hist: patch %s refused (entries >= 1 and 3 * t * h * w * 255^2 < 2^31)" % (tuple(patch),))
    return int(nb)


def patch_proj_hist(vol_u8, patch, dirs_i8, stride=(1, 1, 1)):
    """Histograms of the integer projections of every patch of a volume on P directions (hpvg_patchproj_hist_u8, i8 matrix
    cores): vol is a uint8 device tensor [T,H,W,3] or [H,W,3], dirs an int8 device tensor [P, D] with entries in {-1, 0, +1},
    D = 3 * t * h * w of the patch.  Returns int32 [P, NB], NB = 256 D + 1: hist[p][b] = the number of patches of the strided
    grid with sum_k dirs[p][k] * (byte[k] - 128) == b - 128 D.  Exact; every row sums to the patch count."""
    (v,), _ = _patch_volumes("patch_proj_hist", (("vol", vol_u8),))
    pa, st = _triple(patch, "patch", "patch_proj_hist"), _triple(stride, "stride", "patch_proj_hist")
    NB = patch_proj_bins(patch)
    D = (NB - 1) // 256
    if dirs_i8.dtype != torch.int8 or dirs_i8.dim() != 2 or dirs_i8.shape[0] < 1 or dirs_i8.shape[1] != D:
        raise RuntimeError("patch_proj_hist: dirs must be int8 [P, %d] with P >= 1 for patch %s, got %s %s"
                           % (D, tuple(pa), dirs_i8.dtype, tuple(dirs_i8.shape)))
    dirs = _c(dirs_i8)
    worst = int(dirs.to(torch.int16).abs().max())
    if worst > 1:
        raise RuntimeError("patch_proj_hist: dirs entries must be -1, 0 or +1, got one of magnitude %d" % worst)
    if not vol_u8.is_cuda or not dirs_i8.is_cuda or vol_u8.device != dirs_i8.device:
        raise RuntimeError("patch_proj_hist: vol on %s, dirs on %s; both must be on one MI355X device" % (vol_u8.device, dirs_i8.device))
    P = dirs.shape[0]
    g = tuple(v.shape[:3])
    if call("hpvg_patchproj_ws_bytes", *g, pa, st, 1) == 0:
        raise RuntimeError("patch_proj_hist: vol %s, patch %s, stride %s refused (patch larger than the volume, or a stride < 1)"
                           % (g, tuple(pa), tuple(st)))
    chunk = max(1, PATCH_PROJ_HIST_CAP_BYTES // (4 * NB))
    if chunk >= 128:
        chunk = chunk // 128 * 128
    hist = torch.empty(P, NB, dtype=torch.int32, device=v.device)
    for p0 in range(0, P, chunk):
        n = min(chunk, P - p0)
        nbytes = call("hpvg_patchproj_ws_bytes", *g, pa, st, n)
        ws = _scratch(nbytes, v.device)
        call("hpvg_patchproj_hist_u8", ptr(v), *g, pa, st, ptr(dirs[p0:p0 + n]), n, ptr(hist[p0:p0 + n]), *ws, stream())
    return hist


def hist_w1(histA, Na, histB, Nb):
    """num[p] = sum_b |Nb * cA_p(b) - Na * cB_p(b)| over the cumulative counts of two patch_proj_hist results [P, NB]
    (hpvg_hist_w1_i32): Na * Nb times the 1-D Wasserstein-1 distance of the two projection distributions, int64 [P], exact.
    Na / Nb are the patch counts of the two volumes."""
    for name, h in (("histA", histA), ("histB", histB)):
        if h.dtype != torch.int32 or h.dim() != 2:
            raise RuntimeError("hist_w1: %s must be int32 [P, NB], got %s %s" % (name, h.dtype, tuple(h.shape)))
    if histA.shape != histB.shape:
        raise RuntimeError("hist_w1: histA %s and histB %s must have one shape" % (tuple(histA.shape), tuple(histB.shape)))
    if not histA.is_cuda or histA.device != histB.device:
        raise RuntimeError("hist_w1: histA on %s, histB on %s; both must be on one MI355X device" % (histA.device, histB.device))
    a, b = _c(histA), _c(histB)
    P, NB = a.shape
    num = torch.empty(P, dtype=torch.int64, device=a.device)
    call("hpvg_hist_w1_i32", ptr(a), int(Na), ptr(b), int(Nb), int(P), int(NB), ptr(num), stream())
    return num


def scalar_log_append_(scalars, table, cursor):
    """Append (*scalars[0], ..., *scalars[K-1]) to row cursor % capacity of `table` [capacity][K] and advance the device int
    `cursor` (hpvg_scalar_log_append_f32: one single-wave kernel; captured into a graph it appends on every replay).
    `scalars`: fp32 device tensors of one element each, or (tensor, element index) pairs."""
    from .lib import LOG_MAX_K, ScalarPtrs
    K = len(scalars)
    capacity, k_tab = table.shape
    if not 1 <= K <= LOG_MAX_K or k_tab != K:
        raise RuntimeError("scalar_log_append_: %d scalars for a table of %d columns (at most %d)" % (K, k_tab, LOG_MAX_K))
    src = ScalarPtrs()
    for k, s in enumerate(scalars):
        t, i = s if isinstance(s, tuple) else (s, 0)
        if t.dtype != torch.float32 or not t.is_cuda or not 0 <= i < t.numel():
            raise RuntimeError("scalar_log_append_: column %d is not an fp32 device scalar" % k)
        src.p[k] = t.data_ptr() + 4 * i
    call("hpvg_scalar_log_append_f32", src, K, ptr(table), int(capacity), ptr(cursor), stream())


NOISE_STREAM_BASE = 1 << 31


class noise_stream:
    """Draws made inside `with ops.noise_stream(device):` use call indices from NOISE_STREAM_BASE (top bit set) up, so their
    Philox keys (seed, device iteration, call index) never equal a train iteration's, whose call indices count from 0.  On
    exit the host call index is put back.  torch's CPU / CUDA generators and python's `random` are not touched: previews
    and samples drawn between train iterations leave the data order, the CPU alpha draws and the flips where they were."""

    def __init__(self, device=None, base=NOISE_STREAM_BASE):
        if not base & NOISE_STREAM_BASE:
            raise ValueError("noise_stream: the base call index must have its top bit set")
        self.device = torch.device(device if device is not None else "cuda")
        self.base = base

    def __enter__(self):
        self._st = _rng(self.device)
        self._saved = self._st.call
        self._st.call = self.base
        return self

    def __exit__(self, *exc):
        self._st.call = self._saved
        return False
