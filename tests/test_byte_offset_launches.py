"""Launches of the byte-tensor kernels on tensors at any BYTE offset, inside guard bands (tests/offset_buf.py).

The other suites hand csrc/patchnn.hip, patchmatch.inl, patchnn_prdc.inl and the two byte kernels of frames.hip fresh
allocations.  Their callers do not: evaluate.py walks `for smp in samples_dev`, and sample i of a [N,T,H,W,3] uint8 array starts
i*T*H*W*3 bytes in - an odd address whenever T*H*W and i are odd; ops._patch_volumes asks for contiguity only.  The contract at
the top of include/hpvg.h says a uint8 / int8 tensor argument may have any byte alignment and nothing outside [p, p + n) is read or
written; this module enforces it.

Common rule (that of tests/test_offset_launches.py, in bytes).  Every launch runs with all tensors at offset 0 in guard bands
(the base), with each byte tensor in turn 1, 2, 3, 7 and 13 bytes past a 16-byte boundary, with every tensor at 1, and with the
4-byte side arguments (nn, d2, score, selection lists, weights, radii, histograms, counts: offset_buf.embed / out_like, NaN or -1
around inputs, sentinel bits in outputs) together at 1, 2 and 3 elements.  Every placement runs TWICE: byte inputs between
guards of 0x00 and then of 0xFF, byte outputs pre-filled - guards and payload - with 0x5A and then 0xA5.  After each run every
guard is bit-intact and every output EQUALS the exact numpy restatement (tests/patch_ref.py, patchmatch_ref.py, patchwrap_ref.py,
prdc_ref.py, nnf_chunks_ref.py, volresize_ref.py, oracle/frames.py): a byte read outside the tensor that reaches a result cannot
pass both fills, a byte never stored differs between the two sentinels.  Outputs the C ABI takes by pointer are ours, so every
launch calls the library directly.  No tolerance appears in this module except for the fp32 frame tensor in non-quantised mode,
which keeps the bound of tests/test_frames.py (and is bit-equal to its own base launch at every offset).

After its sweep every workspace-using launch runs once more after launch_common.fill_workspaces(ops) - every workspace byte
0xFF - and must reproduce its base result bit for bit.

The last test is the producer itself: arr[1] of a [2,T,H,W,3] device array with T*H*W odd against arr[1].clone(), through every
ops.patch_* wrapper.

The module prints the number of launches and how many of them were compared by equality."""
import ctypes
import time

import numpy as np
import pytest
import torch

import launch_common as LC
import nnf_chunks_ref as NR
import offset_buf as OB
import patch_ref as PR
import patchmatch_ref as PM
import patchwrap_ref as PW
import prdc_ref as PD
import volresize_ref as VR

pytestmark = pytest.mark.gpu

DEV = "cuda"
I3 = ctypes.c_int * 3
ONE = (1, 1, 1)
U8, I8, I32, F32 = torch.uint8, torch.int8, torch.int32, torch.float32
_COUNT = {"launches": 0, "equal": 0, "tolerance": 0, "reruns": 0, "producer": 0}
_T0 = [None]


@pytest.fixture(scope="module")
def ops():
    import hp_vae_gan_amd  # noqa: F401
    from hp_vae_gan_amd import ops as _ops
    _T0[0] = time.time()
    yield _ops
    torch.cuda.synchronize()
    print("\nbyte-offset launches: %d launches, %d compared by equality with the exact restatement, %d with the frame tensor's "
          "bound; %d reruns on a 0xFF workspace and %d producer pairs, all bit for bit; %.1f s" % (
              _COUNT["launches"], _COUNT["equal"], _COUNT["tolerance"], _COUNT["reruns"], _COUNT["producer"], time.time() - _T0[0]))


@pytest.fixture(scope="module")
def hplib(ops):
    from hp_vae_gan_amd import lib as _hplib
    _hplib.load()
    return _hplib


def _rand(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, size=tuple(shape) + (3,), dtype=np.uint8)


def _weights(n, seed):
    return (0.25 + 3.75 * np.random.default_rng(seed).random(n)).astype(np.float32)      # [0.25, 4): every product normal


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _geom(a):
    """(T, H, W) of a uint8 [T,H,W,3] volume or [H,W,3] image (T = 1)."""
    return tuple(a.shape[:3]) if a.ndim == 4 else (1,) + tuple(a.shape[:2])


# ------------------------------------------------------------------------------------------------ the common rule
def _is_byte(dtype):
    return dtype in (U8, I8)


def _configs(byte, four):
    yield "base", {}
    for n in byte:
        for off in OB.BYTE_OFFSETS[1:]:
            yield "%s@%d" % (n, off), {n: off}
    yield "all@1", {n: 1 for n in byte + four}
    if four:
        for off in OB.OFFSETS[1:]:
            yield "words@%d" % off, {n: off for n in four}


def _place(ins, outs, offs, k, guards):
    T = {}
    for n, t in ins.items():
        if t is None:
            T[n] = None
        elif _is_byte(t.dtype):
            T[n] = OB.embed_u8(t, offs.get(n, 0), OB.BYTE_FILLS[k])
        else:
            T[n] = OB.embed(t, offs.get(n, 0), guard=guards.get(n))
    for n, (shape, dtype) in outs.items():
        if _is_byte(dtype):
            T[n] = OB.out_like_u8(shape, offs.get(n, 0), OB.BYTE_SENTINELS[k], device=DEV, dtype=dtype)
        else:
            T[n] = OB.out_like(shape, dtype, offs.get(n, 0), guard=guards.get(n), device=DEV)
    return T


def _same_bits(a, b):
    if a.dtype == F32:
        return torch.equal(a.contiguous().view(I32), b.contiguous().view(I32))
    return torch.equal(a, b)


def _equals(got, want):
    """got (device tensor) equals the restatement `want` (numpy): integers by value, fp32 bit for bit."""
    want = np.asarray(want)
    if tuple(got.shape) != want.shape:
        return False
    if got.dtype == F32:
        assert want.dtype == np.float32
        return torch.equal(got.cpu().contiguous().view(I32), torch.from_numpy(np.ascontiguousarray(want).view(np.int32)))
    return torch.equal(got.cpu().to(torch.int64), torch.from_numpy(np.ascontiguousarray(want).astype(np.int64)))


def bsweep(ops, what, ins, outs, run, want, uses_ws=False, guards=None):
    """The common rule for one launch.  ins: {name: device tensor or None}; outs: {name: (shape, dtype)}; run(T) launches on the
    placed tensors and may return further results ({name: tensor}: outputs that must stay 8-byte aligned); want: {name: numpy
    restatement, or a function of the result that asserts a bound}.  Returns the base launch's results (clones)."""
    guards = guards or {}
    byte = [n for n, t in ins.items() if t is not None and _is_byte(t.dtype)] + [n for n, (_, d) in outs.items() if _is_byte(d)]
    four = [n for n, t in ins.items() if t is not None and not _is_byte(t.dtype)] + [n for n, (_, d) in outs.items() if not _is_byte(d)]
    base = None
    exact = all(not callable(w) for w in want.values())
    for label, offs in _configs(byte, four):
        for k in (0, 1):
            T = _place(ins, outs, offs, k, guards)
            for n in byte:
                assert T[n].data_ptr() % 16 == offs.get(n, 0) % 16
            extra = run(T) or {}
            torch.cuda.synchronize()
            tag = "%s [%s, guards %#04x, sentinel %#04x]" % (what, label, OB.BYTE_FILLS[k], OB.BYTE_SENTINELS[k])
            for n, t in ins.items():
                if t is not None:
                    assert OB.guards_intact(T[n]), tag + ": the guard band of input %s was written" % n
            res = {}
            for n, (_, dtype) in outs.items():
                if _is_byte(dtype):
                    assert OB.guards_intact(T[n]), tag + ": a guard band around the output %s was written" % n
                else:
                    OB.assert_written(T[n], tag + " output " + n)
                res[n] = T[n]
            res.update(extra)
            for n, w in want.items():
                if callable(w):
                    w(res[n], tag + ": " + n)
                else:
                    assert _equals(res[n], w), tag + ": %s differs from the exact restatement" % n
            if base is None:
                base = {n: t.clone() for n, t in res.items()}
            else:
                for n, t in base.items():
                    assert _same_bits(res[n], t), tag + ": %s differs from the base launch" % n
            _COUNT["launches"] += 1
            _COUNT["equal" if exact else "tolerance"] += 1
    if uses_ws:
        LC.fill_workspaces(ops)
        T = _place(ins, outs, {}, 0, guards)
        extra = run(T) or {}
        torch.cuda.synchronize()
        res = {n: T[n] for n in outs}
        res.update(extra)
        for n, t in base.items():
            assert _same_bits(res[n], t), "%s: %s differs after the workspace was filled with 0xFF" % (what, n)
        _COUNT["launches"] += 1
        _COUNT["reruns"] += 1
    return base


# ================================================================================================ exact search
# (name, q, r, patch): case 1 - D = 54 padded to 64, Nq = 189 (two ragged row tiles), Nr = 112 (less than one tile); case 2 - a
# volume of 315 bytes (not a multiple of 4), D = 75 padded to 128; an image
NN_CASES = [
    ("d54", (4, 9, 11), (3, 10, 9), (2, 3, 3)),
    ("d75", (3, 5, 7), (3, 5, 7), (1, 5, 5)),
    ("image", (9, 11), (10, 9), (1, 3, 3)),
]


def _nn_case(name):
    i = [c[0] for c in NN_CASES].index(name)
    _, qs, rs, patch = NN_CASES[i]
    return _rand(qs, 300 + 2 * i), _rand(rs, 301 + 2 * i), patch


@pytest.mark.parametrize("name", [c[0] for c in NN_CASES])
def test_patchnn_plain_weighted_subset(ops, hplib, name):
    q, r, patch = _nn_case(name)
    qg, rg = _geom(q), _geom(r)
    pa, one = I3(*patch), I3(*ONE)
    counts = (ctypes.c_int * 3)()
    hplib.call("hpvg_patchnn_counts", *qg, *rg, pa, one, one, counts)
    Nq, Nr, D = counts[0], counts[1], counts[2]
    if name == "d54":
        assert (Nq, Nr, D) == (189, 112, 54)
    elif name == "d75":
        assert D == 75 and q.size == 315 and q.size % 4 == 3
    grid = tuple(qg[a] - patch[a] + 1 for a in range(3))
    p, st = hplib.ptr, hplib.stream
    qd, rd = _dev(q), _dev(r)
    io = {"d2": (grid, I32), "nn": (grid, I32)}

    def ws_plain(T):
        return ops._scratch(hplib.call("hpvg_patchnn_ws_bytes", *qg, *rg, pa, one, one), T["q"].device)

    def plain(T):
        hplib.call("hpvg_patchnn_u8", p(T["q"]), *qg, p(T["r"]), *rg, pa, one, one, p(T["d2"]), p(T["nn"]), *ws_plain(T), st())

    d2, nn = PR.brute(q, r, patch)
    bsweep(ops, "patchnn " + name, {"q": qd, "r": rd}, io, plain, {"d2": d2, "nn": nn}, uses_ws=True)

    w = _weights(Nr, 310)

    def weighted(T):
        hplib.call("hpvg_patchnn_weighted_u8", p(T["q"]), *qg, p(T["r"]), *rg, pa, one, one, p(T["w"]), p(T["score"]), p(T["nn"]),
                   *ws_plain(T), st())

    score, wnn = PR.brute_weighted(q, r, w, patch)
    bsweep(ops, "patchnn_weighted " + name, {"q": qd, "r": rd, "w": _dev(w)}, {"score": (grid, F32), "nn": (grid, I32)}, weighted,
           {"score": score, "nn": wnn}, uses_ws=True)

    # the subset search: both lists (ragged lengths), either list alone, both null
    rng = np.random.default_rng(311)
    qsel = np.sort(rng.choice(Nq, size=max(1, (Nq * 3) // 7), replace=False)).astype(np.int32)
    rsel = np.sort(rng.choice(Nr, size=max(1, (Nr * 5) // 11), replace=False)).astype(np.int32)
    assert len(qsel) != len(rsel) or Nq < 4
    lists = [(qsel, rsel), (qsel, None), (None, rsel)] + ([(None, None)] if name == "d54" else [])
    for qs_, rs_ in (lists if name != "image" else lists[:1]):
        nq, nr = (-1 if qs_ is None else len(qs_)), (-1 if rs_ is None else len(rs_))

        def subset(T):
            ws = ops._scratch(hplib.call("hpvg_patchnn_subset_ws_bytes", *qg, *rg, pa, one, one, nq, nr), T["q"].device)
            hplib.call("hpvg_patchnn_subset_u8", p(T["q"]), *qg, p(T["r"]), *rg, pa, one, one, p(T["qsel"]), max(nq, 0), p(T["rsel"]),
                       max(nr, 0), p(T["d2"]), p(T["nn"]), *ws, st())

        sd2, snn = PR.brute_subset(q, r, patch, qs_, rs_)
        if qs_ is None and rs_ is None:
            assert np.array_equal(sd2, d2) and np.array_equal(snn, nn)
        bsweep(ops, "patchnn_subset %s (%s, %s)" % (name, nq, nr), {"q": qd, "r": rd, "qsel": _dev(qs_), "rsel": _dev(rs_)}, io, subset,
               {"d2": sd2, "nn": snn}, uses_ws=True)


# ================================================================================================ PatchMatch
# pw = 3: a line of 9 bytes, two words and a tail of one; pw = 4: whole words.  Query grids 3 x 8 x 10 and 2 x 10 x 34: no multiple
# of the 8 x 32 tile (the second has two tiles along x and along y).  pt = 64 / 68 need 64 * 10 * 104 + 8 and 68 * 9 * 108 + 8
# bytes of LDS, more than the 65536 the kernel has: the query is read from global memory.
PM_CASES = {
    "pw3": ((4, 10, 12), (3, 9, 17), (2, 3, 3)),
    "pw4": ((3, 11, 37), (2, 9, 21), (2, 2, 4)),
    "global_pw3": ((66, 5, 6), (65, 4, 5), (64, 3, 3)),
    "global_pw4": ((70, 4, 7), (69, 3, 6), (68, 2, 4)),
}


def _pm_lds_bytes(patch):
    pt, ph, pw = patch
    return pt * (8 + ph - 1) * (((32 + pw - 1) * 3 + 3) & ~3) + 8


@pytest.mark.parametrize("name", list(PM_CASES))
def test_patchmatch_plain_weighted_init_wrap(ops, hplib, name):
    qs, rs, patch = PM_CASES[name]
    assert (_pm_lds_bytes(patch) > 65536) == name.startswith("global")
    k = list(PM_CASES).index(name)
    q, r = _rand(qs, 320 + 2 * k), _rand(rs, 321 + 2 * k)
    qg, rg = _geom(q), _geom(r)
    grid = tuple(qg[a] - patch[a] + 1 for a in range(3))
    rgrid = tuple(rg[a] - patch[a] + 1 for a in range(3))
    assert grid[1] % 8 or grid[2] % 32
    Nq, Nr = int(np.prod(grid)), int(np.prod(rgrid))
    w = _weights(Nr, 330 + k)
    init = np.random.default_rng(331 + k).integers(0, Nr, size=Nq).astype(np.int32)
    init[::5], init[2::5] = -3, Nr + 17                 # out of range on both sides: clamped
    pa = I3(*patch)
    iters, seed = 2, 11
    p, st = hplib.ptr, hplib.stream
    qd, rd = _dev(q), _dev(r)
    combos = [(None, None), (w, init)] + ([(None, init), (w, None)] if name == "pw3" else [])
    flags = [(None, None)] + ([((1, 0, 1), (0, 1, 1))] if name in ("pw3", "global_pw4") else [])
    for qwrap, rwrap in flags:
        for wt, ini in combos:
            def run(T):
                ws = ops._scratch(hplib.call("hpvg_patchmatch_ws_bytes", *qg, *rg, pa), T["q"].device)
                if qwrap is None:
                    hplib.call("hpvg_patchmatch_u8", p(T["q"]), *qg, p(T["r"]), *rg, pa, p(T["w"]), p(T["init"]), iters, seed, p(T["d2"]),
                               p(T["nn"]), p(T.get("score")), *ws, st())
                else:
                    hplib.call("hpvg_patchmatch_wrap_u8", p(T["q"]), *qg, p(T["r"]), *rg, pa, I3(*qwrap), I3(*rwrap), p(T["w"]),
                               p(T["init"]), iters, seed, p(T["d2"]), p(T["nn"]), p(T.get("score")), *ws, st())

            if qwrap is None:
                d2, nn, score = PM.patch_match_ref(q, r, patch, iters, seed, wt, ini)
            else:
                d2, nn, score = PW.patch_match_wrap_ref(q, r, patch, iters, seed, wt, ini, qwrap, rwrap)
            outs = {"d2": (grid, I32), "nn": (grid, I32)}
            want = {"d2": d2, "nn": nn}
            if wt is not None:
                outs["score"] = (grid, F32)
                want["score"] = score
            bsweep(ops, "patchmatch %s wrap=%s weights=%s init=%s" % (name, qwrap is not None, wt is not None, ini is not None),
                   {"q": qd, "r": rd, "w": _dev(wt), "init": _dev(ini)}, outs, run, want, uses_ws=True)


# ================================================================================================ vote, mask count
def test_patch_vote_and_vote_wrap(ops, hplib):
    """v, fallback and out as byte tensors, nn as int32; a strided grid with an uncovered tail (W: starts 0, 3, 6 of 11) and some
    nn = -1 (and some past Nr); then the vote onto a ring."""
    v, fb, patch, qstride, rstride = _rand((3, 6, 7), 340), _rand((4, 9, 11), 341), (2, 3, 3), (1, 2, 3), (1, 1, 2)
    vg, og = _geom(v), _geom(fb)
    c3 = (ctypes.c_long * 3)()
    hplib.call("hpvg_patch_vote_counts", *og, *vg, I3(*patch), I3(*qstride), I3(*rstride), c3)
    Nq, Nr, uncovered = c3[0], c3[1], c3[2]
    assert uncovered > 0
    nn = np.random.default_rng(342).integers(0, Nr, size=Nq).astype(np.int32)
    nn[::7], nn[3::11] = -1, Nr
    p, st = hplib.ptr, hplib.stream

    def vote(T):
        hplib.call("hpvg_patch_vote_u8", p(T["v"]), *vg, p(T["nn"]), *og, I3(*patch), I3(*qstride), I3(*rstride), p(T["fallback"]),
                   p(T["out"]), st())

    want, cnt = PR.vote_ref(v, nn, patch, fb, qstride, rstride)
    assert int((cnt == 0).sum()) >= uncovered
    bsweep(ops, "patch_vote", {"v": _dev(v), "nn": _dev(nn), "fallback": _dev(fb)}, {"out": (fb.shape, U8)}, vote, {"out": want})

    wrap = (1, 0, 1)
    grid = PW.periodic_grid(og, patch, wrap)
    Nq = grid[0] * grid[1] * grid[2]
    nn = np.random.default_rng(343).integers(0, Nr, size=Nq).astype(np.int32)
    nn[::7] = -1

    def vote_wrap(T):
        hplib.call("hpvg_patch_vote_wrap_u8", p(T["v"]), *vg, p(T["nn"]), *og, I3(*patch), I3(*rstride), I3(*wrap), p(T["fallback"]),
                   p(T["out"]), st())

    want, _ = PW.vote_wrap_ref(v, nn, patch, fb, wrap, rstride)
    bsweep(ops, "patch_vote_wrap", {"v": _dev(v), "nn": _dev(nn), "fallback": _dev(fb)}, {"out": (fb.shape, U8)}, vote_wrap, {"out": want})


def test_patch_mask_count(ops, hplib):
    mask = (np.random.default_rng(350).random((4, 9, 11)) < 0.3).astype(np.uint8) * np.random.default_rng(351).integers(
        1, 256, size=(4, 9, 11)).astype(np.uint8)
    assert mask.ndim == 3 and (mask == 0).any() and (mask > 1).any()
    p, st = hplib.ptr, hplib.stream
    for patch, stride in (((2, 3, 3), ONE), ((2, 3, 3), (1, 2, 3)), ((1, 5, 5), ONE)):
        want = PR.count_ref(mask, patch, stride)

        def run(T):
            hplib.call("hpvg_patch_mask_count_u8", p(T["mask"]), *mask.shape, I3(*patch), I3(*stride), p(T["count"]), st())

        bsweep(ops, "patch_mask_count %s %s" % (patch, stride), {"mask": _dev(mask)}, {"count": (want.shape, I32)}, run, {"count": want})


# ================================================================================================ precision / recall searches
@pytest.mark.parametrize("k", [1, 3])
def test_patchknn_self_and_ball_count(ops, hplib, k):
    q, r, patch = _nn_case("d54")
    qg, rg = _geom(q), _geom(r)
    pa, one = I3(*patch), I3(*ONE)
    p, st = hplib.ptr, hplib.stream
    want = PD.ref_knn_self(q, patch, k)

    def knn(T):
        ws = ops._scratch(hplib.call("hpvg_patchknn_self_ws_bytes", *qg, pa, one, k), T["vol"].device)
        hplib.call("hpvg_patchknn_self_u8", p(T["vol"]), *qg, pa, one, k, p(T["kth"]), *ws, st())

    bsweep(ops, "patchknn_self k=%d" % k, {"vol": _dev(q)}, {"kth": (want.shape, I32)}, knn, {"kth": want}, uses_ws=True)

    radius = PD.ref_knn_self(r, patch, k)[..., k - 1].astype(np.int32)          # the radii evaluate --prdc uses
    count = PD.ref_ball_count(q, r, radius, patch)
    assert 0 < int((count > 0).sum()) and int(count.max()) > 0

    def ball(T):
        ws = ops._scratch(hplib.call("hpvg_patch_ball_count_ws_bytes", *qg, *rg, pa, one, one), T["q"].device)
        hplib.call("hpvg_patch_ball_count_u8", p(T["q"]), *qg, p(T["r"]), *rg, pa, one, one, p(T["radius"]), p(T["count"]), *ws, st())

    bsweep(ops, "patch_ball_count k=%d" % k, {"q": _dev(q), "r": _dev(r), "radius": _dev(radius.reshape(-1))},
           {"count": (count.shape, I32)}, ball, {"count": count}, uses_ws=True)


# ================================================================================================ sliced Wasserstein
def test_patchproj_hist_then_hist_w1(ops, hplib):
    """Volume and int8 directions as byte tensors, P = 130 (two direction tiles, the second ragged); then hpvg_hist_w1_i32 on
    the int32 histograms of two volumes at 4-byte offsets, its 64-bit `num` in an allocation of its own (8-byte aligned)."""
    q, r, patch = _nn_case("d54")
    D, P = 54, 130
    NB = 256 * D + 1
    S = np.random.default_rng(360).integers(-1, 2, size=(P, D), dtype=np.int8)
    S[~S.any(1), 0] = 1
    p, st = hplib.ptr, hplib.stream
    pa, one = I3(*patch), I3(*ONE)
    assert hplib.call("hpvg_patchproj_bins", pa) == NB
    g = _geom(q)
    hA, Na = PR.ref_hist(q, patch, S)

    def run(T):
        ws = ops._scratch(hplib.call("hpvg_patchproj_ws_bytes", *g, pa, one, P), T["vol"].device)
        hplib.call("hpvg_patchproj_hist_u8", p(T["vol"]), *g, pa, one, p(T["dirs"]), P, p(T["hist"]), *ws, st())

    bsweep(ops, "patchproj_hist", {"vol": _dev(q), "dirs": _dev(S)}, {"hist": ((P, NB), I32)}, run, {"hist": hA}, uses_ws=True,
           guards={"hist": 2 * NB})       # two rows of the histogram per side
    hB, Nb = PR.ref_hist(r, patch, S)
    P6 = 6
    hA, hB = np.ascontiguousarray(hA[:P6]), np.ascontiguousarray(hB[:P6])
    want = np.array(PR.ref_num(hA, Na, hB, Nb), np.int64)

    def w1(T):
        num = torch.full((P6,), -1, dtype=torch.int64, device=DEV)
        assert num.data_ptr() % 8 == 0
        hplib.call("hpvg_hist_w1_i32", p(T["histA"]), Na, p(T["histB"]), Nb, P6, NB, p(num), st())
        return {"num": num}

    bsweep(ops, "hist_w1", {"histA": _dev(hA), "histB": _dev(hB)}, {}, w1, {"num": want}, guards={"histA": 64, "histB": 64})


# ================================================================================================ chunks of a field
def test_nnf_chunks_at_4_byte_offsets(ops, hplib):
    q, r, patch = _nn_case("d54")
    d2, nn = PR.brute(q, q[:3, :, :9], patch)            # a field with copied regions: the key volume is a crop of the query
    grid, rgrid = nn.shape, (2, 7, 7)
    nn = nn.astype(np.int32)
    nn[0, 0, :3] = -1
    d2 = d2.astype(np.int32)
    max_d2 = int(np.median(d2))
    p, st = hplib.ptr, hplib.stream
    for use_d2 in (False, True):
        labels, sizes, stats = NR.ref_chunks(nn, rgrid, ONE, ONE, d2 if use_d2 else None, max_d2 if use_d2 else None)
        assert stats[0] > 0 and stats[4] > 1                # some patches kept, and a copied region among them

        def run(T):
            out = torch.full((6,), -1, dtype=torch.int64, device=DEV)
            hplib.call("hpvg_nnf_chunks_i32", p(T["nn"]), p(T["d2"]), max_d2 if use_d2 else 0, I3(*grid), I3(*rgrid), I3(*ONE), I3(*ONE),
                       p(T["labels"]), p(T["sizes"]), p(out), st())
            return {"stats": out}

        bsweep(ops, "nnf_chunks d2=%s" % use_d2, {"nn": _dev(nn), "d2": _dev(d2) if use_d2 else None},
               {"labels": (grid, I32), "sizes": (grid, I32)}, run, {"labels": labels, "sizes": sizes, "stats": stats})


# ================================================================================================ frames.hip
def _video_u8_ref(x):
    """write_video's conversion, the truncating rule tests/test_programs_gpu.py checks: uint8(trunc(clamp((x + 1) * 127.5)))
    with the add and the multiply rounded separately in fp32, [B,C,T,H,W] -> [B,T,H,W,C]."""
    x = x.astype(np.float32)
    u8 = np.trunc(np.clip((x + np.float32(1)) * np.float32(127.5), 0, 255)).astype(np.uint8)
    return np.ascontiguousarray(u8.transpose(0, 2, 3, 4, 1))


@pytest.mark.parametrize("C", [3, 1])
@pytest.mark.parametrize("W", [257, 5])
def test_video_to_u8(ops, hplib, C, W):
    """fp32 input at 4-byte offsets, byte output at byte offsets; W = 257 crosses the kernel's chunk of a row, W = 5 does not;
    values on and next to the 256 level boundaries, both infinities."""
    B, T, H = 2, 2, 3
    rng = np.random.default_rng(370 + C + W)
    x = (rng.random((B, C, T, H, W)) * 2.4 - 1.2).astype(np.float32)
    lv = (np.arange(256, dtype=np.float32) / np.float32(127.5) - np.float32(1)).astype(np.float32)
    special = np.concatenate([lv, np.nextafter(lv, np.float32(np.inf)), np.nextafter(lv, np.float32(-np.inf)),
                              np.array([np.inf, -np.inf], np.float32)])
    pos = rng.permutation(x.size)[:min(x.size // 2, special.size)]
    x.reshape(-1)[pos] = special[:pos.size]
    p, st = hplib.ptr, hplib.stream

    def run(T_):
        hplib.call("hpvg_video_to_u8_f32", p(T_["x"]), p(T_["out"]), B, C, T, H, W, st())

    bsweep(ops, "video_to_u8 C=%d W=%d" % (C, W), {"x": _dev(x)}, {"out": ((B, T, H, W, C), U8)}, run, {"out": _video_u8_ref(x)})


@pytest.mark.parametrize("quantize", [1, 0])
def test_frames_resize_norm(ops, hplib, quantize):
    """Byte source at byte offsets, fp32 clip tensor in out_like; with and without hflip; windows that end on the clip's LAST
    frame (nothing past it may be read: the 0xFF run would show it), down- and upsizing."""
    from oracle import frames as OF
    N, H, W = 5, 7, 9
    frames = np.random.default_rng(380).integers(0, 256, size=(N, H, W, 3), dtype=np.uint8)
    p, st = hplib.ptr, hplib.stream
    for first, step, count, h, w, hflip in ((2, 1, 3, 5, 6, 0), (0, 2, 3, 10, 13, 1), (4, 1, 1, 7, 9, 1)):
        assert first + (count - 1) * step == N - 1
        want = OF.clip_tensor(frames, first, step, count, h, w, bool(hflip), bool(quantize))

        def run(T):
            hplib.call("hpvg_frames_resize_norm_u8_f32", p(T["src"]), p(T["dst"]), N, H, W, first, step, count, h, w, hflip, quantize, st())

        def bound(got, tag):                             # tests/test_frames.py: fp32 tap weights, ~1e-3 of a uint8 level
            assert np.abs(got.double().cpu().numpy() - want).max() < 1e-5, tag

        if quantize:
            assert want.dtype == np.float32
        bsweep(ops, "frames_resize_norm q=%d %s" % (quantize, (first, step, count, h, w, hflip)), {"src": _dev(frames)},
               {"dst": ((3, count, h, w), F32)}, run, {"dst": want if quantize else bound})


# ================================================================================================ the exact resize
def test_volume_resize(ops, hplib):
    src = _rand((3, 5, 7), 390)
    p, st = hplib.ptr, hplib.stream
    for size in ((2, 4, 5), (4, 7, 9), (3, 5, 4)):
        want = VR.resize(src, size)

        def run(T):
            hplib.call("hpvg_volume_resize_u8", p(T["src"]), *src.shape[:3], p(T["out"]), *size, st())

        bsweep(ops, "volume_resize %s" % (size,), {"src": _dev(src)}, {"out": (tuple(size) + (3,), U8)}, run, {"out": want})


# ================================================================================================ the producer itself
def test_every_patch_wrapper_on_a_sample_of_a_batch(ops):
    """arr[1] of a [2,T,H,W,3] device array with T*H*W odd starts an odd number of bytes into the allocation - what evaluate.py's
    `for smp in samples_dev` hands every wrapper.  Each ops.patch_* result on it equals the result on arr[1].clone(), bit for
    bit."""
    T, H, W = 3, 5, 7
    assert (T * H * W) % 2 == 1
    arr = _dev(np.random.default_rng(400).integers(0, 256, size=(2, T, H, W, 3), dtype=np.uint8))
    ref = _dev(_rand((3, 6, 8), 401))
    mask = _dev((np.random.default_rng(402).random((2, T, H, W)) < 0.3).astype(np.uint8))
    smp, own = arr[1], arr[1].clone()
    assert smp.is_contiguous() and smp.data_ptr() % 2 == 1 and own.data_ptr() % 16 == 0
    assert mask[1].data_ptr() % 2 == 1
    patch = (2, 3, 3)
    Nq, Nr, D = ops.patch_nn_counts((T, H, W), tuple(ref.shape[:3]), patch)
    Ns = ops.patch_nn_counts((T, H, W), (T, H, W), patch)[0]
    g = torch.Generator(device=DEV).manual_seed(403)
    w_ref = torch.rand(Nr, generator=g, device=DEV) * 3.75 + 0.25
    w_smp = torch.rand(Ns, generator=g, device=DEV) * 3.75 + 0.25
    init = torch.randint(0, Nr, (Nq,), generator=g, device=DEV, dtype=torch.int64).to(I32)
    qsel = torch.arange(0, Nq, 2, device=DEV, dtype=I32)
    rsel = torch.arange(1, Nr, 3, device=DEV, dtype=I32)
    rad_ref = torch.randint(20000, 200000, (Nr,), generator=g, device=DEV, dtype=torch.int64).to(I32)
    rad_smp = torch.randint(20000, 200000, (Ns,), generator=g, device=DEV, dtype=torch.int64).to(I32)
    nn_vote = torch.randint(-1, Ns, (Nr,), generator=g, device=DEV, dtype=torch.int64).to(I32)
    dirs = torch.randint(-1, 2, (7, D), generator=g, device=DEV, dtype=torch.int64).to(I8)
    calls = {
        "patch_nn (query)": lambda s: ops.patch_nn(s, ref, patch),
        "patch_nn (ref)": lambda s: ops.patch_nn(ref, s, patch),
        "patch_nn_weighted (query)": lambda s: ops.patch_nn_weighted(s, ref, w_ref, patch),
        "patch_nn_weighted (ref)": lambda s: ops.patch_nn_weighted(ref, s, w_smp, patch),
        "patch_match (query)": lambda s: ops.patch_match(s, ref, patch, 2, 5, w_ref, init),
        "patch_match (ref)": lambda s: ops.patch_match(ref, s, patch, 2, 5),
        "patch_match wrap (query)": lambda s: ops.patch_match(s, ref, patch, 2, 5, qwrap=(1, 0, 1), rwrap=(0, 1, 0)),
        "patch_match wrap (ref)": lambda s: ops.patch_match(ref, s, patch, 2, 5, qwrap=(0, 1, 0), rwrap=(1, 0, 1)),
        "patch_nn_subset (query)": lambda s: ops.patch_nn_subset(s, ref, patch, qsel, rsel),
        "patch_nn_subset (ref)": lambda s: ops.patch_nn_subset(ref, s, patch, rsel[:5], qsel),
        "patch_knn_self": lambda s: (ops.patch_knn_self(s, patch, 3),),
        "patch_ball_count (query)": lambda s: (ops.patch_ball_count(s, ref, rad_ref, patch),),
        "patch_ball_count (ref)": lambda s: (ops.patch_ball_count(ref, s, rad_smp, patch),),
        "patch_vote (values)": lambda s: (ops.patch_vote(s, nn_vote, patch, tuple(ref.shape[:3]), ref),),
        "patch_vote (fallback)": lambda s: (ops.patch_vote(ref, init, patch, (T, H, W), s),),
        "patch_vote wrap (fallback)": lambda s: (ops.patch_vote(ref, init.repeat(3)[:T * (H - 2) * W].contiguous(), patch,
                                                                (T, H, W), s, wrap=(1, 0, 1)),),
        "patch_proj_hist": lambda s: (ops.patch_proj_hist(s, patch, dirs),),
        "volume_resize_u8": lambda s: (ops.volume_resize_u8(s, (2, 4, 5)),),
    }
    for name, fn in calls.items():
        a = fn(smp)
        b = fn(own)
        torch.cuda.synchronize()
        assert len(a) == len(b)
        for x, y in zip(a, b):
            assert x.dtype == y.dtype and _same_bits(x, y), "%s on arr[1] differs from the same call on arr[1].clone()" % name
        _COUNT["producer"] += 1
    a, b = ops.patch_mask_count(mask[1], patch), ops.patch_mask_count(mask[1].clone(), patch)
    assert torch.equal(a, b)
    _COUNT["producer"] += 1
    assert torch.equal(smp, own)                          # nothing wrote into the sample
