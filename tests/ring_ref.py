"""Float64 restatements of the ring features of `generate` (--size, --wrap), written from their definitions in include/hpvg.h
and hp_vae_gan_amd/generate.py, not from the kernels (tests/test_generate_ring_host.py, tests/test_generate_ring_gpu.py).

  ring_pad_ref        out[c, t, y, x] = x[c, mod(t - pt, T), mod(y - ph, H), mod(x - pw, W)]
  ring_resize_ref     separable linear resize: align-corners on a plain axis, source coordinate o S / O on a ring axis
  level_sizes_ref     the pyramid of another finest size at the trained ratios, halves rounded up
  ring_conv_ref       np.pad(mode="wrap") on the ring axes, zeros elsewhere, then the direct VALID convolution
  ring_conv_route_ref the same conv the way modules/_nets.Conv runs it: ring pad, zero-padded 'same' conv, crop
  generator_ring_ref  the HP-VAE-GAN sampling path (decoder, tanh, per level resize, noise, block, tanh residual)

Seeded defects.  The keyword `defect` of a function computes it wrongly in one named way; the host test requires that each
defect is told from the clean function on the shapes the GPU tests use - a case that cannot tell them apart checks nothing."""
import numpy as np
import torch
import torch.nn.functional as F


# ------------------------------------------------------------------------------------------------------------------ pad
def ring_pad_ref(x, pad, defect=None):
    """x: [..., T, H, W] array -> [..., T + 2 pt, H + 2 ph, W + 2 pw], float64.  defect 'sign': mod(i + p, side)."""
    x = np.asarray(x, dtype=np.float64)
    out = x
    for k, p in enumerate(pad):
        ax = x.ndim - 3 + k
        side = x.shape[ax]
        p = int(p)
        assert p >= 0
        i = np.arange(side + 2 * p)
        src = np.mod(i + p, side) if defect == "sign" else np.mod(i - p, side)
        out = np.take(out, src, axis=ax)
    return out


# --------------------------------------------------------------------------------------------------------------- resize
def _axis_taps(S, O, ring, defect=None):
    """(i0, i1, f) of the O outputs of one axis, float64 weights 1 - f and f.
    defects: 'i1_unwrapped' - the last sample of a ring repeats itself instead of reaching the first;
             'ac_rule' - a ring axis computed by the align-corners rule."""
    o = np.arange(O)
    if ring and defect != "ac_rule":
        p = o * S
        i0 = p // O
        f = (p % O) / float(O)
        i1 = np.minimum(i0 + 1, S - 1) if defect == "i1_unwrapped" else (i0 + 1) % S
        return i0, i1, f
    src = o * ((S - 1) / float(O - 1)) if O > 1 else np.zeros(O)
    i0 = np.minimum(np.floor(src).astype(np.int64), S - 1)
    i1 = np.minimum(i0 + 1, S - 1)
    return i0, i1, src - i0


def ring_resize_ref(x, size, wrap, defect=None, with_scale=False):
    """x: [..., Ts, Hs, Ws] -> [..., To, Ho, Wo] float64; wrap: (wt, wh, ww).  with_scale: also A, the largest |x| among the
    8 taps each output reads (the scale of the project's rule |got - ref| <= 1e-5 A)."""
    y = np.asarray(x, dtype=np.float64)
    A = np.abs(y)
    for k in range(3):
        ax = y.ndim - 3 + k
        i0, i1, f = _axis_taps(y.shape[ax], int(size[k]), bool(wrap[k]), defect)
        sh = [1] * y.ndim
        sh[ax] = -1
        f = f.reshape(sh)
        y = (1.0 - f) * np.take(y, i0, axis=ax) + f * np.take(y, i1, axis=ax)
        A = np.maximum(np.take(A, i0, axis=ax), np.take(A, i1, axis=ax))
    return (y, A) if with_scale else y


# ---------------------------------------------------------------------------------------------------------- level sizes
def level_sizes_ref(trained, size):
    """Per level l and axis a: s_l[a] where size[a] equals the trained finest side, else max(1, round_half_up(s_l[a] size[a] /
    s_L[a])) in exact integers."""
    fine = [int(v) for v in trained[-1]]
    out = []
    for s in trained:
        q = []
        for a, want in enumerate(size):
            if int(want) == fine[a]:
                q.append(int(s[a]))
            else:
                num, den = 2 * int(s[a]) * int(want) + fine[a], 2 * fine[a]
                q.append(max(1, num // den))
        out.append(q)
    return out


# ----------------------------------------------------------------------------------------------------------------- conv
def _valid_conv(x64, w64):
    return F.conv3d(x64, w64) if x64.dim() == 5 else F.conv2d(x64, w64)


def _torch_pad(x64, ring, p, circular):
    """Pad every spatial axis by p: ring axes circularly (np.pad wrap) when `circular`, everything else with zeros."""
    a = x64.numpy()
    nd = a.ndim - 2
    wrap_w = [(0, 0), (0, 0)] + [(p, p) if (ring[k] and circular) else (0, 0) for k in range(nd)]
    zero_w = [(0, 0), (0, 0)] + [(0, 0) if (ring[k] and circular) else (p, p) for k in range(nd)]
    a = np.pad(a, wrap_w, mode="wrap") if p else a
    a = np.pad(a, zero_w, mode="constant")
    return torch.from_numpy(np.ascontiguousarray(a))


def ring_conv_ref(x, w, b, ring):
    """The circular convolution on the axes flagged in `ring` (one flag per spatial axis), zero padding on the others:
    np.pad(mode='wrap') / zeros by K // 2, then the direct valid convolution, in float64 -> (y, A); A is the same conv of
    |x|, |w|, |b|, the error scale of tests/conv_ref.py."""
    x64, w64 = x.detach().double().cpu(), w.detach().double().cpu()
    p = int(w.shape[2]) // 2
    y = _valid_conv(_torch_pad(x64, ring, p, True), w64)
    A = _valid_conv(_torch_pad(x64.abs(), ring, p, True), w64.abs())
    if b is not None:
        b64 = b.detach().double().cpu().view(1, -1, *([1] * (x.dim() - 2)))
        y = y + b64
        A = A + b64.abs()
    return y, A.float()


def ring_conv_route_ref(x, w, b, ring, defect=None):
    """ring_conv_ref the way the module computes it: the ring axes padded circularly by K // 2 (ring_pad_ref), the zero-padded
    'same' conv of the padded volume, the ring axes cropped back.  defects: 'sign' (of the pad), 'crop' (off by one)."""
    x64, w64 = x.detach().double().cpu(), w.detach().double().cpu()
    nd = x.dim() - 2
    p = int(w.shape[2]) // 2
    pad3 = [0] * (3 - nd) + [p * int(bool(f)) for f in ring]
    a = x64.numpy() if nd == 3 else x64.numpy()[:, :, None]
    xp = torch.from_numpy(np.ascontiguousarray(ring_pad_ref(a, pad3, defect="sign" if defect == "sign" else None)))
    xp = xp if nd == 3 else xp[:, :, 0]
    y = _valid_conv(_torch_pad(xp, [0] * nd, p, False), w64)
    if b is not None:
        y = y + b.detach().double().cpu().view(1, -1, *([1] * nd))
    for k in range(nd):
        c = pad3[3 - nd + k]
        if c:
            y = y.narrow(2 + k, c + (1 if defect == "crop" else 0), x.shape[2 + k])
    return y.contiguous()


# ------------------------------------------------------------------------------------------------------------ generator
def _bn_lrelu(r, gamma, beta, eps=1e-5, slope=0.2):
    dims = [0] + list(range(2, r.dim()))
    mean = r.mean(dim=dims, keepdim=True)
    var = ((r - mean) ** 2).mean(dim=dims, keepdim=True)     # the biased variance of the batch, as train-mode BatchNorm
    sh = [1, -1] + [1] * (r.dim() - 2)
    h = (r - mean) / torch.sqrt(var + eps) * gamma.view(sh) + beta.view(sh)
    return torch.where(h > 0, h, slope * h)


def _stack(seq, x, ring):
    """head ConvBlock + blocks + tail conv of modules/_nets._seven_conv_stack on float64 copies of its parameters."""
    d = {k: v.detach().double().cpu() for k, v in seq.state_dict().items()}
    names = [n for n, _ in seq.named_children()]
    for n in names:
        if n == "tail":
            x, _ = ring_conv_ref(x, d["tail.weight"], d["tail.bias"], ring)
        else:
            r, _ = ring_conv_ref(x, d[n + ".conv.weight"], d[n + ".conv.bias"], ring)
            x = _bn_lrelu(r, d[n + ".norm.weight"], d[n + ".norm.bias"])
    return x


def generator_ring_ref(netG, noise_init, noise_amps, sizes, ring, noises):
    """Float64 CPU forward of GeneratorHPVAEGAN's sampling path (mode 'rand', noise_init given): vae_out = tanh(decoder(z));
    per level l = 1 .. L: up = resize(x, sizes[l]) (ring_resize_ref), up_noisy = up + amp_l * noise where the level injects
    noise (3-D: from the first GAN level on; 2-D: every level), x = tanh(block(up_noisy) + up).  BatchNorm uses batch
    statistics.  sizes: the level shapes 0 .. L; ring: one flag per spatial axis (all zero: zero padding and the align-corners
    resize); noises: the recorded level noises in the order they were drawn."""
    nd = noise_init.dim() - 2
    ring = [int(f) for f in ring]
    assert len(ring) == nd and list(noise_init.shape[2:]) == [int(s) for s in sizes[0]]
    wrap3 = [0] * (3 - nd) + ring
    x = torch.tanh(_stack(netG.decoder, noise_init.detach().double().cpu(), ring))
    noises = list(noises)
    for idx, block in enumerate(netG.body):
        size = [int(s) for s in sizes[idx + 1]]
        a = x.numpy() if nd == 3 else x.numpy()[:, :, None]
        up = torch.from_numpy(np.ascontiguousarray(ring_resize_ref(a, [1] * (3 - nd) + size, wrap3)))
        up = up if nd == 3 else up[:, :, 0]
        up_noisy = up
        if nd == 2 or netG.opt.vae_levels <= idx + 1:
            nz = noises.pop(0).detach().double().cpu()
            assert tuple(nz.shape) == tuple(up.shape), (tuple(nz.shape), tuple(up.shape))
            up_noisy = up + float(noise_amps[idx + 1]) * nz
        x = torch.tanh(_stack(block, up_noisy, ring) + up)
    assert not noises, "%d recorded noises were not used" % len(noises)
    return x
