"""The library's noise stream restated in numpy (tests/test_noise_stream_host.py, tests/test_noise_stream_gpu.py).

Every N(0,1) and U[0,1) draw of training and sampling comes from one device function (csrc/elementwise.hip: philox4x32_10,
philox_normal4): Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123 library
publishes known-answer vectors) followed by Box-Muller.  Element i of a draw of n values is value i % 4 of block q = i // 4:

    words(q) = philox4x32_10(counter = (q & 0xFFFFFFFF, q >> 32, call_id, iter), key = (seed & 0xFFFFFFFF, seed >> 32))
    uniform  : (word >> 8) * 2^-24                                  exact in fp32, [0, 1)
    normal   : u = ((float)(word >> 8) + 0.5f) * 2^-24   in fp32;   (ra cos a, ra sin a, rb cos b, rb sin b) with
               ra = sqrt(-2 ln u_x), a = 2pi_f32 * u_y, rb = sqrt(-2 ln u_z), b = 2pi_f32 * u_w

The u of the normal is NOT confined to the open interval (0, 1): k + 0.5 has no fp32 representation for k >= 2^23 and rounds
to even, so k = 2^24 - 1 gives u = 1.0 exactly (radius sqrt(-0): both values of the pair are signed zeros; as an angle it is
fp32 2pi) and k = 2^23 gives 0.5 exactly.  The smallest u is 2^-25 (k = 0), the largest |n| sqrt(-2 ln 2^-25) = 5.887.

The reference takes u and the angle as the kernel forms them - each is ONE correctly rounded fp32 operation on exact inputs,
so numpy's float32 gives the same bits - and evaluates log, sqrt, cos and sin in float64.  What the rule below then measures
is the device's logf / sqrtf / sincosf and the two products, against the scale ra of the pair:

    every value finite,   |got - ref| <= tau * ra,   and where ra == 0 the value is +-0 exactly.

Numpy only; nothing here needs a GPU.  The constants are module globals so that the host test can seed defects into them."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57          # multipliers on c0 and c2
W0, W1 = 0x9E3779B9, 0xBB67AE85          # key increments (golden ratio, sqrt(3) - 1)
ROUNDS = 10
MASK = 0xFFFFFFFF
TWO_PI_F32 = np.float32(6.283185307179586)
INV_2_24 = np.float32(2.0 ** -24)
MAX_ABS = float(np.sqrt(-2.0 * np.log(2.0 ** -25)))   # 5.887: the radius of k = 0

# Random123's known-answer vectors for philox4x32-10: (counter, key, output)
KAT = (
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((MASK, MASK, MASK, MASK), (MASK, MASK), (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
)

# (what, call_id, word, k): with seed 0, iteration 0, block 0 the 24-bit value of `word` (0..3 = x, y, z, w) is k.  Found by a
# one-off search over call_id < 2^26 (philox4x32_10 below, in chunks); test_noise_stream_host.py re-derives every line.
K_TOP, K_HALF = 0xFFFFFF, 1 << 23
EDGE_KEYS = (
    ("x: u = 1.0, radius 0", 1205178, 0, K_TOP),
    ("x: u = 2^-25, largest radius", 33008474, 0, 0),
    ("y: angle = fp32 2pi", 10174669, 1, K_TOP),
    ("y: smallest angle", 9373564, 1, 0),
    ("z: u = 1.0, radius 0", 12895450, 2, K_TOP),
    ("z: u = 2^-25, largest radius", 18189822, 2, 0),
    ("w: angle = fp32 2pi", 10475606, 3, K_TOP),
    ("w: smallest angle", 32098591, 3, 0),
    ("x: k = 2^23, u = 0.5 exactly", 12125520, 0, K_HALF),
    ("w: k = 2^23, angle = fp32 pi", 28584014, 3, K_HALF),
)


def _u64(v):
    return np.asarray(v, dtype=np.uint64)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """The four output words (uint64 arrays holding 32-bit values) of counter (c0..c3) under key (k0, k1); arguments are
    scalars or arrays that broadcast, each < 2^32."""
    c0, c1, c2, c3, k0, k1 = (_u64(v) for v in (c0, c1, c2, c3, k0, k1))
    mask, s32 = np.uint64(MASK), np.uint64(32)
    for _ in range(ROUNDS):
        p0 = np.uint64(M0) * c0          # 32 x 32 -> 64 bits: never wraps
        p1 = np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & mask, (p0 >> s32) ^ c3 ^ k1, p0 & mask
        k0 = (k0 + np.uint64(W0)) & mask
        k1 = (k1 + np.uint64(W1)) & mask
    return c0, c1, c2, c3


def stream_words(n, seed, call_id, it, first_block=0):
    """uint64 [ceil(n / 4), 4]: the words of blocks q = first_block .. first_block + ceil(n / 4) - 1 of the stream
    (seed: 64 bits, call_id: 32 bits, it: the device int's value, taken as uint32)."""
    seed, call_id, it = int(seed), int(call_id), int(it) & MASK
    assert 0 <= seed < 1 << 64 and 0 <= call_id <= MASK and n >= 1
    q = np.arange(first_block, first_block + (int(n) + 3) // 4, dtype=np.uint64)
    words = philox4x32_10(q & np.uint64(MASK), q >> np.uint64(32), call_id, it, seed & MASK, seed >> 32)
    return np.stack([np.broadcast_to(w, q.shape) for w in words], axis=1)


def uniform_from_words(words, n):
    """float32 [n]: (word >> 8) * 2^-24, exact."""
    return ((words >> np.uint64(8)).astype(np.float32) * INV_2_24).reshape(-1)[:n]


def unit(words):
    """float32, the kernel's u of a word: ((float)(word >> 8) + 0.5f) * 2^-24, each step rounded to fp32."""
    return ((words >> np.uint64(8)).astype(np.float32) + np.float32(0.5)) * INV_2_24


def normal_from_words(words, n):
    """(float64 [n] reference, float64 [n] scale): Box-Muller of (x, y) and of (z, w) per block; the scale of a value is the
    radius of its pair."""
    u = unit(words)
    angle = (TWO_PI_F32 * u[:, 1::2]).astype(np.float64)        # one fp32 product, as the kernel forms it
    radius = np.sqrt(-2.0 * np.log(u[:, 0::2].astype(np.float64))) + 0.0   # + 0.0: sqrt(-0.0) = -0.0 becomes 0
    ref = np.stack([radius * np.cos(angle), radius * np.sin(angle)], axis=2)   # [nq, pair, (cos, sin)]
    scale = np.stack([radius, radius], axis=2)
    return ref.reshape(-1)[:n], scale.reshape(-1)[:n]


def uniform_ref(n, seed, call_id, it):
    return uniform_from_words(stream_words(n, seed, call_id, it), n)


def normal_ref(n, seed, call_id, it):
    return normal_from_words(stream_words(n, seed, call_id, it), n)


def normal_ratio(got, ref, scale):
    """max_i |got_i - ref_i| / scale_i of a float32 result; infinite where a value is not finite or, at scale 0, not +-0."""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == ref.shape == scale.shape, (got.dtype, got.shape, ref.shape, scale.shape)
    d = np.abs(got.astype(np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(scale > 0, d / scale, np.where(d == 0, 0.0, np.inf))
    ratio = np.where(np.isfinite(got) & ~np.isnan(ratio), ratio, np.inf)
    return float(ratio.max())
