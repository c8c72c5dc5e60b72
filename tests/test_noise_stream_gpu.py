"""The library's noise stream on the device against the numpy restatement of tests/philox_ref.py (whose Philox reproduces
Random123's published vectors, tests/test_noise_stream_host.py): hpvg_uniform_f32 bit for bit, hpvg_normal_f32 and the noise
of hpvg_upsample_linear_ac_noise_f32 element by element against float64 Box-Muller,

    every value finite,   |got - ref| <= TAU * ra  (ra: the radius of the value's pair),   +-0 exactly where ra == 0,

with TAU = conv_ref.TAU = 1e-5.  Kernels are launched through the C ABI with an explicit (seed, call_id, iteration pointer).

Sizes: every n % 4 tail, one thread, one block +- 1 element, several grid-stride steps with a ragged last block - each at
every 4-byte offset inside guard bands of both fills -, and one draw above the 4096-block cap.  Keys: seeds with and without
a high word, call indices up to 2^32 - 1, the iteration as a device int (negative included) and as NULL; the committed edge
keys that hit u = 1.0 (radius 0), the largest radius and both ends of the angle.  Then the python layer (ops.normal_ /
ops.uniform_ follow torch.manual_seed, the call index advances by one, rng_next_iteration, noise_stream) and the stream
allocation of two real train iterations: every draw of an iteration has its own call index.

Worst |got - ref| / ra measured on an MI355X (printed at module end): see DESIGN.md, "Noise stream"."""
import numpy as np
import pytest
import torch

import conv_ref as R
import ew_ref as E
import offset_buf as OB
import philox_ref as P
from helpers import hip_opt, load_golden

pytestmark = pytest.mark.gpu

DEV = "cuda"
TAU = R.TAU
KERNELS = ("hpvg_normal_f32", "hpvg_uniform_f32")
SIZES = (1, 2, 3, 4, 5, 1023, 1024, 1025, 4 * 1024 * 3 + 2)
N_CAPPED = 4 * (4096 * 1024) + 4 * 1024 * 3 + 1      # ew_blocks caps the grid at 4096 blocks of 256 threads x 4 blocks of 4 values
_STATS = {}
_CAPPED = {}


@pytest.fixture(scope="module")
def ops():
    import hp_vae_gan_amd  # noqa: F401
    from hp_vae_gan_amd import ops as _ops
    yield _ops
    _CAPPED.clear()
    if _STATS:
        print("\nhpvg_normal_f32 / fused noise: worst |got - ref| / ra per case (tau %.0e):" % TAU)
        for k, v in sorted(_STATS.items()):
            print("  %-28s %.3e" % (k, v))


@pytest.fixture(scope="module")
def hplib(ops):
    from hp_vae_gan_amd import lib as _lib
    _lib.load()
    return _lib


def _iter_dev(value):
    return None if value is None else torch.tensor([value], dtype=torch.int32, device=DEV)


def _launch(hplib, name, out, seed, call_id, it):
    """`it`: None (a NULL pointer) or the value of the device int."""
    dev = _iter_dev(it)
    hplib.call(name, hplib.ptr(out), out.numel(), seed, call_id, hplib.ptr(dev), hplib.stream())
    torch.cuda.synchronize()
    return out


def _check(name, got, seed, call_id, it, what, case):
    """One draw against the reference of its kernel; returns the host copy."""
    got = got.detach().reshape(-1).cpu().numpy()
    n, it = got.size, it or 0
    if name == "hpvg_uniform_f32":
        assert float(got.min()) >= 0.0 and float(got.max()) < 1.0, what + ": a uniform outside [0, 1)"
        ref = P.uniform_ref(n, seed, call_id, it)
        bad = np.nonzero(got.view(np.uint32) != ref.view(np.uint32))[0]
        assert bad.size == 0, "%s: %d of %d uniforms differ, first at %d: got %.9g, ref %.9g" % (
            what, bad.size, n, bad[0], got[bad[0]], ref[bad[0]])
    else:
        _check_normal(got, *P.normal_ref(n, seed, call_id, it), what, case)
    return got


def _check_normal(got, ref, scale, what, case):
    r = P.normal_ratio(got, ref, scale)
    _STATS[case] = max(_STATS.get(case, 0.0), r)
    if not r <= TAU:
        with np.errstate(divide="ignore", invalid="ignore"):
            e = np.abs(got.astype(np.float64) - ref) / scale
        i = int(np.argmax(np.where(np.isfinite(got), np.nan_to_num(e, nan=np.inf), np.inf)))
        raise AssertionError("%s: |got - ref| / ra = %.3e > tau %.0e at element %d: got %.9g, ref %.9g, ra %.9g" % (
            what, r, TAU, i, got[i], ref[i], scale[i]))


# ------------------------------------------------------------------------------------------------ sizes, tails, guard bands
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", KERNELS)
def test_sizes_at_every_offset_inside_guard_bands(ops, hplib, name, n):
    """The draw of n values lands at 4-byte offsets 0..3 of a guarded buffer - guards and payload the sentinel NaN, then
    guards the plain NaN around a zero payload -, equals the reference each time and leaves every guard word as it was: the
    n % 4 tail stores neither spill nor go missing."""
    seed, call_id, it = (1 << 32) + 7, 5, 3
    first = None
    for off in OB.OFFSETS:
        for fill in ("sentinel", "nan"):
            what = "%s n=%d offset %d, %s guards" % (name, n, off, fill)
            if fill == "sentinel":
                out = OB.out_like((n,), torch.float32, off, device=DEV)
            else:
                out = OB.embed(torch.zeros(n), off, device=DEV)
            assert OB.residue(out) == 4 * off
            _launch(hplib, name, out, seed, call_id, it)
            assert OB.guards_intact(out), what + ": a guard band around the output was written"
            if fill == "sentinel":
                OB.assert_written(out, what)
            if first is None:
                first = torch.from_numpy(_check(name, out, seed, call_id, it, what, "n=%d" % n))
            else:
                assert torch.equal(out.cpu().view(torch.int32), first.view(torch.int32)), what + ": differs from offset 0"


def _capped_words():
    if "w" not in _CAPPED:
        _CAPPED["w"] = P.stream_words(N_CAPPED, (1 << 63) + 11, 9, 2)
    return _CAPPED["w"]


@pytest.mark.parametrize("name", KERNELS)
def test_draw_above_the_block_cap(ops, hplib, name):
    """16.8 M values (67 MB): the grid is capped at 4096 blocks, so every thread makes a fifth grid-stride step or none, and
    the last block of values is one element long.  The whole draw against the host reference (its words computed once)."""
    out = torch.full((N_CAPPED + 64,), float("nan"), device=DEV)
    got = _launch(hplib, name, out[:N_CAPPED], (1 << 63) + 11, 9, 2).cpu().numpy()
    assert bool(torch.isnan(out[N_CAPPED:]).all()), name + ": wrote past n"
    del out
    w = _capped_words()
    what = "%s n=%d" % (name, N_CAPPED)
    if name == "hpvg_uniform_f32":
        assert float(got.min()) >= 0.0 and float(got.max()) < 1.0, what + ": a uniform outside [0, 1)"
        assert np.array_equal(got.view(np.uint32), P.uniform_from_words(w, N_CAPPED).view(np.uint32)), what
    else:
        _check_normal(got, *P.normal_from_words(w, N_CAPPED), what, "n=%d" % N_CAPPED)
        assert float(np.abs(got).max()) <= P.MAX_ABS * (1 + TAU)


# ------------------------------------------------------------------------------------------------ keys
S32, S64, C31, C32, IMAX = 1 << 32, (1 << 64) - 1, 1 << 31, (1 << 32) - 1, (1 << 31) - 1
KEYS = [(s, 0, 0) for s in (0, 1, S32, S32 + 1, S64)] + [(0, c, 0) for c in (1, C31, C32)] + [(0, 0, i) for i in (1, IMAX, -1)] + [
    (1, 1, 1), (1, 0, 1), (S32, 1, 0), (S32, C31, 0), (S32, C32, 1), (S32 + 1, 0, 1), (S32 + 1, C31, IMAX), (S64, C32, -1),
    (S64, 1, IMAX), (1, C31, -1)]
N_KEYS = 4099


def test_keys_are_what_the_reference_says_and_all_different(ops, hplib):
    """Seeds 0, 1, 2^32, 2^32 + 1, 2^64 - 1 x call indices 0, 1, 2^31, 2^32 - 1 x iterations 0, 1, 2^31 - 1, -1 (a device
    int), crossed sparsely: each draw equals its reference - so the seed's high word, the call index and the iteration each
    sit in their own counter / key word - and no two of the streams are equal.  A NULL iteration pointer is iteration 0."""
    assert len(KEYS) == len(set(KEYS)) == 21 and P.MASK == C32
    from hp_vae_gan_amd import ops as hops
    assert hops.NOISE_STREAM_BASE == C31
    for name in KERNELS:
        seen = {}
        for seed, call_id, it in KEYS:
            out = _launch(hplib, name, torch.empty(N_KEYS, device=DEV), seed, call_id, it)
            got = _check(name, out, seed, call_id, it, "%s key (%#x, %#x, %d)" % (name, seed, call_id, it), "keys")
            seen[(seed, call_id, it)] = got.tobytes()
        assert len(set(seen.values())) == len(KEYS), name + ": two keys gave the same stream"
        for seed, call_id in ((0, 0), (S32 + 1, C31)):
            out = _launch(hplib, name, torch.empty(N_KEYS, device=DEV), seed, call_id, None)
            want = seen.get((seed, call_id, 0)) or _launch(hplib, name, torch.empty(N_KEYS, device=DEV), seed, call_id, 0).cpu().numpy().tobytes()
            assert out.cpu().numpy().tobytes() == want, name + ": iter = NULL differs from iteration 0"
            _check(name, out, seed, call_id, None, name + " iter = NULL", "keys")


@pytest.mark.parametrize("what,call_id,word,k", P.EDGE_KEYS, ids=[e[0].split(":")[0] + "-%06x" % e[3] for e in P.EDGE_KEYS])
def test_edge_keys(ops, hplib, what, call_id, word, k):
    """The committed keys whose first block holds an extreme 24-bit value: u = 1.0 must give two exact zeros (sqrt(-0), not
    NaN), k = 0 the largest radius 5.887, the angles 2pi * 2^-25 and fp32 2pi their cos / sin within tau."""
    for it in (None, 0):
        got = _launch(hplib, "hpvg_normal_f32", torch.empty(4, device=DEV), 0, call_id, it).cpu().numpy()
        ref, scale = P.normal_ref(4, 0, call_id, 0)
        _check_normal(got, ref, scale, "edge key %d (%s)" % (call_id, what), "edge keys")
        pair = got[2 * (word // 2):2 * (word // 2) + 2].astype(np.float64)
        if word % 2 == 0 and k == P.K_TOP:
            assert pair.tolist() == [0.0, 0.0], "%s: %s, not two zeros" % (what, pair)
        if word % 2 == 0 and k == 0:
            assert abs(np.hypot(*pair) - P.MAX_ABS) <= TAU * P.MAX_ABS, "%s: pair norm %.9g" % (what, np.hypot(*pair))
        uni = _launch(hplib, "hpvg_uniform_f32", torch.empty(4, device=DEV), 0, call_id, it).cpu().numpy()
        assert uni[word] == k / 2.0 ** 24 and np.array_equal(uni, P.uniform_ref(4, 0, call_id, 0))


# ------------------------------------------------------------------------------------------------ the fused resize + noise kernel
def test_fused_resize_noise_against_the_independent_reference(ops, hplib):
    """hpvg_upsample_linear_ac_noise_f32 at (4, 3, 4, 18, 33) -> (4, 23, 41), first_noisy = 2: yn - y of the noisy samples
    is amp * (the reference normal of the element's flat index) within TAU * amp * ra plus the rounding of the fp32 add,
    TAU * |y|; below first_noisy yn is y bit for bit; y itself against the float64 resize of tests/ew_ref.py."""
    B, C, first_noisy, amp = 4, 3, 2, 0.37
    ins, outs = (4, 18, 33), (4, 23, 41)
    seed, call_id, it = S32 + 3, 4242, 6
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, C, *ins, generator=g).to(DEV)
    y = OB.out_like((B, C) + outs, torch.float32, 1, device=DEV)
    yn = OB.out_like((B, C) + outs, torch.float32, 3, device=DEV)
    it_dev = _iter_dev(it)
    hplib.call("hpvg_upsample_linear_ac_noise_f32", hplib.ptr(x), hplib.ptr(y), hplib.ptr(yn), amp, B * C, C, first_noisy, *ins, *outs,
               seed, call_id, hplib.ptr(it_dev), hplib.stream())
    torch.cuda.synchronize()
    OB.assert_written(y, "fused resize + noise: y")
    OB.assert_written(yn, "fused resize + noise: yn")
    # y against the float64 resize (the plain resize kernel is another compilation of the same sum: its bits may differ)
    R.check(y, *E.resize64(x, outs), "fused resize + noise: y")
    assert torch.equal(yn[:first_noisy], y[:first_noisy]), "noise below first_noisy"
    n = y.numel()
    lo = first_noisy * (n // B)
    y64 = y.cpu().numpy().reshape(-1)[lo:].astype(np.float64)
    yn32 = yn.cpu().numpy().reshape(-1)[lo:]
    assert np.all(np.isfinite(yn32))
    ref, ra = P.normal_ref(n, seed, call_id, it)
    a = float(np.float32(amp))
    err = np.abs(yn32.astype(np.float64) - y64 - a * ref[lo:])
    bound = a * ra[lo:] + np.abs(y64)
    r = float((err / bound).max())
    _STATS["fused resize + noise"] = r
    i = int(np.argmax(err / bound))
    assert r <= TAU, "yn - y against amp * N(0,1): %.3e > tau %.0e at element %d: yn %.9g, y %.9g, amp * ref %.9g" % (
        r, TAU, lo + i, yn32[i], y64[i], a * ref[lo + i])


# ------------------------------------------------------------------------------------------------ the python layer
@pytest.mark.parametrize("seed", [0, (1 << 32) + 5, -3], ids=["0", "2^32+5", "-3"])
def test_ops_draws_follow_manual_seed_and_count_calls(ops, seed):
    """torch.manual_seed(s) then ops.normal_ / ops.uniform_: key (s mod 2^64, call index, device iteration) - a negative seed
    is its two's complement, what torch.initial_seed() & (2^64 - 1) yields -, the call index one up per draw,
    rng_next_iteration back to 0 with the device counter one up, noise_stream from 2^31 and back."""
    dev = torch.device(DEV, torch.cuda.current_device())
    with torch.random.fork_rng(devices=[dev.index]):
        ops._rng_states.clear()
        torch.manual_seed(seed)
        key = seed % (1 << 64)
        assert ops._seed() == key and (seed >= 0 or key == (1 << 64) + seed)
        n = 1025

        def draw(fn, name, call_id, it, what):
            out = fn(torch.empty(n, device=DEV))
            torch.cuda.synchronize()
            _check(name, out, key, call_id, it, "seed %d: %s" % (seed, what), "ops")

        draw(ops.normal_, "hpvg_normal_f32", 0, 0, "first draw")
        st = ops._rng(dev)
        assert st.call == 1 and int(st.iter_dev) == 0 and ops._rng(torch.device(DEV)) is st
        draw(ops.uniform_, "hpvg_uniform_f32", 1, 0, "second draw")
        draw(ops.normal_, "hpvg_normal_f32", 2, 0, "third draw")
        assert st.call == 3
        ops.rng_next_iteration(dev)
        assert st.call == 0 and int(st.iter_dev) == 1
        draw(ops.uniform_, "hpvg_uniform_f32", 0, 1, "first draw of iteration 1")
        draw(ops.normal_, "hpvg_normal_f32", 1, 1, "second draw of iteration 1")
        with ops.noise_stream(dev):
            assert st.call == ops.NOISE_STREAM_BASE == 1 << 31
            draw(ops.normal_, "hpvg_normal_f32", 1 << 31, 1, "first draw under noise_stream")
            draw(ops.uniform_, "hpvg_uniform_f32", (1 << 31) + 1, 1, "second draw under noise_stream")
        assert st.call == 2 and int(st.iter_dev) == 1
        draw(ops.normal_, "hpvg_normal_f32", 2, 1, "draw after noise_stream")
        ops.rng_next_iteration(DEV)
        assert st.call == 0 and int(st.iter_dev) == 2
    ops._rng_states.clear()


@pytest.mark.parametrize("fname", ["step3d_vae_s1.pt", "step3d_gan_s3.pt"])
def test_every_draw_of_a_train_iteration_has_its_own_call_index(ops, monkeypatch, fname):
    """Two eager StageTrainer iterations on the library's own noise (no injected draws): the Philox launches of an iteration
    use call indices 0 .. k - 1 once each - two draws on one index would hand two pyramid levels the same noise - under one
    device iteration value, and the two iterations' values differ."""
    from hp_vae_gan_amd import train as hp_train
    from hp_vae_gan_amd.modules import networks_3d
    fx = load_golden(fname)
    s = fx["scale_idx"]
    ops._rng_states.clear()
    with torch.random.fork_rng(devices=[torch.cuda.current_device()]):
        torch.manual_seed(11)
        opt = hip_opt(fx["opt"], 3, s, DEV)
        netG = networks_3d.GeneratorHPVAEGAN(opt)
        for _ in range(s):
            netG.init_next_stage()
        netG.load_state_dict(fx["G_init"])
        netG.to(DEV)
        netD = None
        if fx["D_init"] is not None:
            netD = networks_3d.WDiscriminator3D(opt)
            netD.load_state_dict(fx["D_init"])
            netD.to(DEV)
        opt.Noise_Amps = list(fx["noise_amps_init"])
        trainer = hp_train.StageTrainer(opt, netG, netD)
        real, real_zero = fx["real"].to(DEV), fx["real_zero"].to(DEV)
        launch = ops._philox_call
        records = []

        def recorder(name, device, *args):
            st = ops._rng(device)
            records[-1].append((name, st.call, int(st.iter_dev)))
            launch(name, device, *args)
            assert st.call == records[-1][-1][1] + 1

        monkeypatch.setattr(ops, "_philox_call", recorder)
        for _ in range(2):
            records.append([])
            trainer.step(real, real_zero)
        torch.cuda.synchronize()
    ops._rng_states.clear()
    iters = []
    for rec in records:
        calls = [c for _, c, _ in rec]
        assert len(rec) >= 2 and calls == list(range(len(rec))), "%s: call indices of one iteration: %s" % (fname, rec)
        assert len(set(i for _, _, i in rec)) == 1, rec
        iters.append(rec[0][2])
    assert iters[0] != iters[1], iters
    # the first iteration also calibrates the noise amplitude, so it draws at least as often as the second
    assert len(records[0]) >= len(records[1])
    names = set(name for name, _, _ in records[1])
    assert "hpvg_normal_f32" in names, records[1]                       # noise_init and the reparameterisation eps
    if netD is not None:
        assert "hpvg_upsample_linear_ac_noise_f32" in names, records[1]   # the level noise of the GAN levels, made in the resize
