"""numpy restatement of hpvg_volume_resize_u8 (include/hpvg.h): the exact antialiased resize of a uint8 volume [T,H,W,3].

Two forms: `resize` builds the three weight matrices and contracts them with one int64 einsum; `resize_loops` is the contract
read aloud, a triple loop over Python ints (arbitrary precision), for the smallest cases."""
import numpy as np


def weights(S, O):
    """int64 [O, S]: w(o, i) = max(0, R - |i (O-1) - o (S-1)|), R = max(O-1, S-1); the identity when S == O."""
    S, O = int(S), int(O)
    if S < 1 or O < 1:
        raise ValueError("weights: sides >= 1, got %d -> %d" % (S, O))
    if S == O:
        return np.eye(S, dtype=np.int64)
    i = np.arange(S, dtype=np.int64)[None, :]
    o = np.arange(O, dtype=np.int64)[:, None]
    R = max(O - 1, S - 1)
    return np.maximum(0, R - np.abs(i * (O - 1) - o * (S - 1)))


def dmax_and_reads(src_size, out_size):
    """(the largest D over the outputs, the largest number of source voxels one output reads), Python ints."""
    d, n = 1, 1
    for S, O in zip(src_size, out_size):
        w = weights(S, O)
        d *= max(int(e) for e in w.sum(1))
        n *= int((w > 0).sum(1).max())
    return d, n


def resize(vol, size):
    """uint8 [T,H,W,3] -> uint8 [*size, 3]: out = (2 N + D) // (2 D), N = sum wt wh ww v, D = (sum wt)(sum wh)(sum ww)."""
    vol = np.asarray(vol)
    assert vol.dtype == np.uint8 and vol.ndim == 4 and vol.shape[3] == 3, (vol.dtype, vol.shape)
    wt, wh, ww = (weights(S, O) for S, O in zip(vol.shape[:3], size))
    assert 511 * dmax_and_reads(vol.shape[:3], size)[0] < 2 ** 63
    N = np.einsum('at,bh,cw,thwk->abck', wt, wh, ww, vol.astype(np.int64), optimize=True)
    D = (wt.sum(1)[:, None, None] * wh.sum(1)[None, :, None] * ww.sum(1)[None, None, :])[..., None]
    out = (2 * N + D) // (2 * D)
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def resize_loops(vol, size):
    """The same in plain loops over Python ints."""
    vol = np.asarray(vol)
    Ts, Hs, Ws = vol.shape[:3]
    To, Ho, Wo = (int(e) for e in size)

    def w(S, O, o, i):
        if S == O:
            return 1 if i == o else 0
        return max(0, max(O - 1, S - 1) - abs(i * (O - 1) - o * (S - 1)))
    out = np.zeros((To, Ho, Wo, 3), np.uint8)
    v = vol.tolist()
    for a in range(To):
        for b in range(Ho):
            for c in range(Wo):
                n, d = [0, 0, 0], 0
                for t in range(Ts):
                    wt = w(Ts, To, a, t)
                    if not wt:
                        continue
                    for h in range(Hs):
                        wth = wt * w(Hs, Ho, b, h)
                        if not wth:
                            continue
                        for x in range(Ws):
                            wx = wth * w(Ws, Wo, c, x)
                            d += wx
                            for k in range(3):
                                n[k] += wx * v[t][h][x][k]
                for k in range(3):
                    out[a, b, c, k] = (2 * n[k] + d) // (2 * d)
    return out
