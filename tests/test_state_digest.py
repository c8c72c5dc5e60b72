"""The state digest's reference (tests/digest_ref.py) on the CPU, and the symbol's declaration and export.

The hand-worked values are the published first outputs of splitmix64 seeded with 0 (Vigna's splitmix64.c: the state advances
by the golden-ratio constant and passes through the finaliser), which are fmix(1 * GOLDEN), fmix(2 * GOLDEN), ...: the
digest's terms for zero words at positions 1, 2, ..."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import digest_ref as dr  # noqa: E402

SPLITMIX64_SEED0 = [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F, 0xF88BB8A8724C81EC]


def test_reference_on_hand_worked_inputs():
    assert dr.digest([]) == 0 and dr.digest([], salt=5) == 0
    assert dr.digest([0]) == 0                                   # fmix(0 * GOLDEN ^ 0) = fmix(0) = 0
    for k, want in enumerate(SPLITMIX64_SEED0, start=1):
        assert dr.digest([0], salt=k) == want, k
        assert dr.digest_int([0], salt=k) == want, k
    assert dr.digest([0, 0, 0]) == (SPLITMIX64_SEED0[0] + SPLITMIX64_SEED0[1]) % (1 << 64)
    assert dr.digest([0] * 5) == sum(SPLITMIX64_SEED0) % (1 << 64)
    # a word is XORed into the low half of the keyed position: position 1 with word w is fmix(GOLDEN ^ w)
    g = 0x9E3779B97F4A7C15
    assert dr.digest([7, 0xFFFFFFFF]) == (dr.fmix_int(7) + dr.fmix_int(g ^ 0xFFFFFFFF)) % (1 << 64)
    # the salt wraps mod 2^64
    assert dr.digest([3], salt=(1 << 64) + 2) == dr.digest([3], salt=2)
    assert dr.digest([3, 4], salt=(1 << 64) - 1) == (dr.digest([3], salt=(1 << 64) - 1) + dr.digest([4], salt=0)) % (1 << 64)


def test_numpy_and_python_int_restatements_agree():
    rng = np.random.default_rng(0)
    for n in (1, 2, 5, 64, 257):
        w = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
        for salt in (0, 1, 12345, (1 << 63) + 9):
            assert dr.digest(w, salt) == dr.digest_int(w.tolist(), salt), (n, salt)


def test_reference_sees_a_flipped_bit_a_swap_and_the_salt():
    rng = np.random.default_rng(1)
    w = rng.integers(0, 1 << 32, size=300, dtype=np.uint64).astype(np.uint32)
    base = dr.digest(w)
    for pos in (0, 1, 150, 299):
        for bit in (0, 13, 31):
            x = w.copy()
            x[pos] ^= np.uint32(1 << bit)
            assert dr.digest(x) != base, (pos, bit)
    for i, j in ((0, 1), (7, 200), (298, 299)):
        assert w[i] != w[j]
        x = w.copy()
        x[i], x[j] = w[j], w[i]
        assert dr.digest(x) != base, (i, j)
    assert dr.digest(w, salt=1) != base and dr.digest(w, salt=300) != base
    # equal words swapped: the same state, the same digest
    x = w.copy()
    x[5] = x[9]
    y = x.copy()
    y[5], y[9] = x[9], x[5]
    assert dr.digest(x) == dr.digest(y)


def test_two_salted_calls_equal_one_call_over_the_concatenation():
    rng = np.random.default_rng(2)
    for n1, n2 in ((1, 1), (3, 70), (64, 5), (257, 1023), (0, 9), (9, 0)):
        a = rng.integers(0, 1 << 32, size=n1, dtype=np.uint64).astype(np.uint32)
        b = rng.integers(0, 1 << 32, size=n2, dtype=np.uint64).astype(np.uint32)
        assert (dr.digest(a, 0) + dr.digest(b, n1)) % (1 << 64) == dr.digest(np.concatenate([a, b])), (n1, n2)
        assert dr.digest_arrays([a, b]) == dr.digest(np.concatenate([a, b]))


def test_words_of_eight_byte_elements_low_word_first():
    a = np.array([0x1122334455667788, -2], dtype=np.int64)
    assert dr.words_of(a).tolist() == [0x55667788, 0x11223344, 0xFFFFFFFE, 0xFFFFFFFF]
    f = np.array([-0.0, np.nan], dtype=np.float32)
    assert dr.words_of(f).tolist() == [0x80000000, 0x7FC00000]
    assert dr.digest_arrays([f, a]) == dr.digest([0x80000000, 0x7FC00000, 0x55667788, 0x11223344, 0xFFFFFFFE, 0xFFFFFFFF])


def test_symbol_is_declared_and_exported():
    import ctypes
    from hp_vae_gan_amd import lib
    assert "hpvg_state_digest_u32" in lib.check_symbols()
    ret, args = lib._SIGNATURES["hpvg_state_digest_u32"]
    assert ret is ctypes.c_int
    assert args == [ctypes.c_void_p, ctypes.c_long, ctypes.c_ulonglong, ctypes.c_void_p, ctypes.c_void_p]
