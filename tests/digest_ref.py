"""numpy uint64 restatement of hpvg_state_digest_u32 (include/hpvg.h): the state digest of snapshot.py.

    digest(words, salt) = sum over i of fmix(((salt + i) * GOLDEN) ^ word[i])   mod 2^64
    fmix(z): z ^= z >> 30; z *= M1; z ^= z >> 27; z *= M2; z ^= z >> 31          (the splitmix64 finaliser)

numpy's uint64 arithmetic wraps mod 2^64, which is the arithmetic asked for.  `words_of` turns an array of a 4-byte or 8-byte
dtype into its 32-bit words (an 8-byte element is two words, low word first: the little-endian memory order)."""
import numpy as np

GOLDEN = np.uint64(0x9E3779B97F4A7C15)
M1 = np.uint64(0xBF58476D1CE4E5B9)
M2 = np.uint64(0x94D049BB133111EB)
MASK = (1 << 64) - 1


def fmix(z):
    z = np.asarray(z, dtype=np.uint64).copy()
    with np.errstate(over="ignore"):
        z ^= z >> np.uint64(30)
        z *= M1
        z ^= z >> np.uint64(27)
        z *= M2
        z ^= z >> np.uint64(31)
    return z


def words_of(a):
    a = np.ascontiguousarray(a)
    if a.dtype.itemsize not in (4, 8):
        raise ValueError("4-byte and 8-byte dtypes only, got %s" % a.dtype)
    return a.reshape(-1).view("<u4")


def digest(words, salt=0):
    """The digest of the uint32 array `words` keyed from position `salt`, a python int in [0, 2^64)."""
    w = np.asarray(words, dtype=np.uint32).reshape(-1).astype(np.uint64)
    if w.size == 0:
        return 0
    with np.errstate(over="ignore"):
        pos = np.arange(w.size, dtype=np.uint64) + np.uint64(int(salt) & MASK)
        terms = fmix((pos * GOLDEN) ^ w)
        return int(np.add.reduce(terms, dtype=np.uint64))


def digest_arrays(arrays):
    """ops.state_digest's rule: each array's salt is the number of words before it."""
    total, salt = 0, 0
    for a in arrays:
        w = words_of(a)
        total = (total + digest(w, salt)) & MASK
        salt += w.size
    return total


def fmix_int(z):
    """fmix on python ints (an independent restatement, for the hand-worked cases)."""
    z &= MASK
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & MASK
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def digest_int(words, salt=0):
    return sum(fmix_int((((salt + i) & MASK) * 0x9E3779B97F4A7C15 & MASK) ^ int(w)) for i, w in enumerate(words)) & MASK
