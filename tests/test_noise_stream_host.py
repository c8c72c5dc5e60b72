"""Host checks (no GPU) behind tests/test_noise_stream_gpu.py: the numpy restatement of the library's noise stream
(tests/philox_ref.py) against Random123's published philox4x32-10 vectors, the committed edge keys re-derived, the two facts
about the kernel's uniforms that its old comment got wrong (u reaches 1.0; it never goes below 2^-25), and the power of the
GPU test's comparison rule: ten defects seeded into a float32 model of the kernel, each of which the rule must reject while
it accepts the model as the kernel is written."""
import numpy as np
import pytest

import conv_ref as R
import philox_ref as P

N = 1 << 18                                   # 2^17 Box-Muller pairs: ~25 of them have u < 2e-4, where a missing + 0.5 shows
KEY = ((1 << 32) + 5, 3, 7)                   # seed with a high word, call index and iteration that differ


def test_known_answer_vectors():
    for counter, key, want in P.KAT:
        got = tuple(int(v) for v in P.philox4x32_10(*counter, *key))
        assert got == want, "philox4x32_10(%s; %s) = %s, published %s" % (
            " ".join("%08x" % v for v in counter), " ".join("%08x" % v for v in key),
            " ".join("%08x" % v for v in got), " ".join("%08x" % v for v in want))
    # arrays give what scalars give
    cols = [np.array([v[0][j] for v in P.KAT], dtype=np.uint64) for j in range(4)]
    keys = [np.array([v[1][j] for v in P.KAT], dtype=np.uint64) for j in range(2)]
    got = np.stack(P.philox4x32_10(*cols, *keys), axis=1)
    assert got.tolist() == [list(v[2]) for v in P.KAT]


def test_stream_words_layout():
    """Counter = (q & 0xFFFFFFFF, q >> 32, call_id, iter as uint32), key = (seed & 0xFFFFFFFF, seed >> 32); element i is word
    i % 4 of block i // 4.  The counter's high word only moves past 2^34 elements: the reference has it, no device test can."""
    seed, call, it = KEY
    w = P.stream_words(9, seed, call, it)
    assert w.shape == (3, 4) and w.dtype == np.uint64 and int(w.max()) <= P.MASK
    for q in range(3):
        assert w[q].tolist() == [int(v) for v in P.philox4x32_10(q, 0, call, it, seed & P.MASK, seed >> 32)]
    hi = P.stream_words(5, seed, call, it, first_block=(3 << 32) + 1)
    assert hi[1].tolist() == [int(v) for v in P.philox4x32_10(2, 3, call, it, 5, 1)]
    assert np.array_equal(P.stream_words(4, 0, 0, -1), P.stream_words(4, 0, 0, P.MASK))      # a device int of -1
    assert np.array_equal(P.stream_words(4, 0, 0, -(1 << 31)), P.stream_words(4, 0, 0, 1 << 31))
    u = P.uniform_ref(9, seed, call, it)
    assert u.dtype == np.float32 and u.shape == (9,)
    assert u.tolist() == [(int(w[i // 4, i % 4]) >> 8) / 2.0 ** 24 for i in range(9)]
    ref, scale = P.normal_ref(9, seed, call, it)
    assert ref.shape == scale.shape == (9,) and ref.dtype == scale.dtype == np.float64
    # the second pair comes from words z, w; a prefix of a longer draw is the shorter draw
    u2, u3 = P.unit(w[:, 2]).astype(np.float64), P.unit(w[:, 3])
    rb, b = np.sqrt(-2 * np.log(u2)), (P.TWO_PI_F32 * u3).astype(np.float64)
    assert np.array_equal(ref[2::4], (rb * np.cos(b))[:2]) and np.array_equal(ref[3::4], (rb * np.sin(b))[:2])
    assert np.array_equal(scale[2::4], rb[:2]) and np.array_equal(scale[3::4], rb[:2])
    assert np.array_equal(P.normal_ref(6, seed, call, it)[0], ref[:6])


def test_interval_of_the_uniforms():
    """uniform: [0, 1 - 2^-24].  The normal's u: [2^-25, 1.0] - k + 0.5 rounds to even from k = 2^23 on, so k = 2^24 - 1
    gives 1.0 and k = 2^23 gives 0.5 - and with it |n| <= sqrt(-2 ln 2^-25) = 5.887, the radius 0 at u = 1."""
    k = np.array([0, 1, (1 << 23) - 1, 1 << 23, (1 << 23) + 1, (1 << 24) - 2, (1 << 24) - 1], dtype=np.uint64)
    words = (k << np.uint64(8)) | np.uint64(0xFF)           # the low 8 bits play no part
    u = P.unit(words)
    assert u.dtype == np.float32
    exact = (k.astype(np.float64) + 0.5) / 2.0 ** 24
    assert u[0] == 2.0 ** -25 and u[1] == exact[1] and u[2] == exact[2]      # below 2^23 nothing rounds
    assert u[3] == 0.5 and u[3] != exact[3] and u[6] == 1.0 and u[5] == 1.0 - 2.0 ** -23 and u[4] == 0.5 + 2.0 ** -23
    assert np.all(np.diff(u.astype(np.float64)) >= 0)
    flat = P.uniform_from_words(words.reshape(1, -1), k.size)
    assert flat[0] == 0.0 and flat[-1] == 1.0 - 2.0 ** -24 and np.array_equal(flat.astype(np.float64), k / 2.0 ** 24)
    assert P.MAX_ABS == pytest.approx(5.8871, abs=1e-4)
    top = np.uint64(P.K_TOP << 8)
    ref, scale = P.normal_from_words(np.array([[top, top, 0, top]], dtype=np.uint64), 4)
    assert scale.tolist() == [0.0, 0.0, P.MAX_ABS, P.MAX_ABS]
    assert ref[0] == 0 and ref[1] == 0 and not np.signbit(scale[0])
    a = float(P.TWO_PI_F32)                                  # fp32 2pi lies 1.7e-7 above 2pi
    assert ref[2] == P.MAX_ABS * np.cos(a) and ref[3] == P.MAX_ABS * np.sin(a) and 0 < ref[3] < 2e-6
    # a whole draw stays inside the bounds
    w = P.stream_words(N, *KEY)
    uu = P.unit(w)
    assert uu.min() >= 2.0 ** -25 and uu.max() <= 1.0
    ref, scale = P.normal_from_words(w, N)
    assert np.all(np.isfinite(ref)) and np.abs(ref).max() <= P.MAX_ABS and np.all(np.abs(ref) <= scale)
    assert abs(ref.mean()) < 5 / np.sqrt(N) and abs(ref.std() - 1) < 5 / np.sqrt(2 * N)


@pytest.mark.parametrize("what,call_id,word,k", P.EDGE_KEYS, ids=[e[0].split(":")[0] + "-%06x" % e[3] for e in P.EDGE_KEYS])
def test_edge_keys_hold_what_they_claim(what, call_id, word, k):
    w = P.stream_words(4, 0, call_id, 0)
    assert w.shape == (1, 4) and int(w[0, word]) >> 8 == k, what
    u = P.unit(w)[0, word]
    ref, scale = P.normal_from_words(w, 4)
    pair = slice(2 * (word // 2), 2 * (word // 2) + 2)
    if k == P.K_HALF:
        assert u == 0.5, what
    elif word % 2 == 0 and k == P.K_TOP:
        assert u == 1.0 and scale[pair].tolist() == [0.0, 0.0] and ref[pair].tolist() == [0.0, 0.0], what
    elif word % 2 == 0:
        assert u == 2.0 ** -25 and scale[pair].tolist() == [P.MAX_ABS] * 2, what
        assert np.hypot(*ref[pair]) == pytest.approx(P.MAX_ABS, rel=1e-15), what
    elif k == P.K_TOP:
        assert P.TWO_PI_F32 * u == P.TWO_PI_F32 and ref[pair][1] > 0, what     # sin of fp32 2pi: + 1.7e-7 * radius
    else:
        assert P.TWO_PI_F32 * u == np.float32(6.283185307179586 * 2.0 ** -25), what
    assert len(set(e[1] for e in P.EDGE_KEYS)) == len(P.EDGE_KEYS)
    assert {(e[2], e[3]) for e in P.EDGE_KEYS} >= {(j, v) for j in range(4) for v in (0, P.K_TOP)}
    assert any(e[3] == P.K_HALF for e in P.EDGE_KEYS)


# ------------------------------------------------------------------------------------------------ the rule and its power
def _model_normal(words, n, unit=P.unit, swap=False):
    """The kernel in numpy float32, operation by operation (philox_normal4): numpy's fp32 log / sqrt / cos / sin stand in for
    the device's."""
    u = unit(words)
    assert u.dtype == np.float32
    with np.errstate(divide="ignore"):
        radius = np.sqrt(np.float32(-2.0) * np.log(u[:, 0::2]))
    angle = P.TWO_PI_F32 * u[:, 1::2]
    c, s = radius * np.cos(angle), radius * np.sin(angle)
    out = np.stack([s, c] if swap else [c, s], axis=2)
    assert out.dtype == np.float32
    return out.reshape(-1)[:n]


def _words(seed=KEY[0], call=KEY[1], it=KEY[2], **kw):
    return P.stream_words(N, seed, call, it, **kw)


def _low24(w):
    return (w & np.uint64(0xFFFFFF)) << np.uint64(8)


def _xy_twice(w):
    w = w.copy()
    w[:, 2:] = w[:, :2]
    return w


def _unit_without_half(words):
    return (words >> np.uint64(8)).astype(np.float32) * P.INV_2_24


# name -> (constants of philox_ref to change, words of the defective stream, keyword arguments of the model, uniform changes too)
DEFECTS = {
    "nine rounds": (dict(ROUNDS=9), _words, {}, True),
    "multipliers swapped": (dict(M0=P.M1, M1=P.M0), _words, {}, True),
    "key increments swapped": (dict(W0=P.W1, W1=P.W0), _words, {}, True),
    "call and iteration words exchanged": ({}, lambda: _words(call=KEY[2], it=KEY[1]), {}, True),
    "seed high word ignored": ({}, lambda: _words(seed=KEY[0] & P.MASK), {}, True),
    "low 24 bits instead of the top 24": ({}, lambda: _low24(_words()), {}, True),
    "sin and cos exchanged": ({}, _words, dict(swap=True), False),
    "second pair fed from (x, y) again": ({}, lambda: _xy_twice(_words()), {}, True),
    "element i from block i / 4 + 1": ({}, lambda: _words(first_block=1), {}, True),
    "u without the + 0.5": ({}, _words, dict(unit=_unit_without_half), False),
}


@pytest.fixture(scope="module")
def correct():
    w = _words()
    ref, scale = P.normal_from_words(w, N)
    return w, ref, scale, P.uniform_from_words(w, N)


def test_rule_accepts_the_kernel_as_written(correct):
    """The float32 model is within tau of the float64 reference - by a factor of ~50 (numpy's libm: 2.1e-7) - and the
    uniform is the same bits."""
    w, ref, scale, uni = correct
    r = P.normal_ratio(_model_normal(w, N), ref, scale)
    print("\nfloat32 model against the float64 reference: worst |got - ref| / ra = %.3e (tau %.0e)" % (r, R.TAU))
    assert r <= R.TAU and r < 1e-6
    assert np.array_equal(P.uniform_ref(N, *KEY), uni) and uni.min() >= 0.0 and uni.max() < 1.0


@pytest.mark.parametrize("name", list(DEFECTS))
def test_rule_rejects_a_seeded_defect(monkeypatch, correct, name):
    consts, make_words, model_kw, moves_uniform = DEFECTS[name]
    _, ref, scale, uni = correct
    for k, v in consts.items():
        monkeypatch.setattr(P, k, v)
    w = make_words()
    monkeypatch.undo()
    got = _model_normal(w, N, **model_kw)
    r = P.normal_ratio(got, ref, scale)
    assert r > R.TAU, "%s: the rule accepts the defective normal stream (worst ratio %.3e)" % (name, r)
    if moves_uniform:
        assert not np.array_equal(P.uniform_from_words(w, N), uni), "%s: the uniform stream is unchanged" % name


def test_rule_on_single_values():
    """Not finite -> rejected; at radius 0 only +-0 passes; elsewhere tau * ra, however small the value itself."""
    ref, scale = np.array([0.0, 0.0, 1e-7, 3.0]), np.array([0.0, 0.0, 3.0, 3.0])
    f = np.float32
    assert P.normal_ratio(np.array([0.0, -0.0, 1e-7, 3.0], dtype=f), ref, scale) < 1e-7
    assert P.normal_ratio(np.array([1e-30, 0.0, 1e-7, 3.0], dtype=f), ref, scale) == np.inf
    assert P.normal_ratio(np.array([np.nan, 0.0, 1e-7, 3.0], dtype=f), ref, scale) == np.inf
    assert P.normal_ratio(np.array([0.0, 0.0, np.nan, 3.0], dtype=f), ref, scale) == np.inf
    assert P.normal_ratio(np.array([0.0, 0.0, 1e-7, np.inf], dtype=f), ref, scale) == np.inf
    assert P.normal_ratio(np.array([0.0, 0.0, 1e-7 + 6e-5, 3.0], dtype=f), ref, scale) == pytest.approx(2e-5, rel=1e-3)
    with pytest.raises(AssertionError):
        P.normal_ratio(np.zeros(4), ref, scale)              # a float64 result is not what a kernel wrote
