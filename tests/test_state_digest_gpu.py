"""hpvg_state_digest_u32 / ops.state_digest on the GPU against tests/digest_ref.py, by equality.

Sizes: 0 (no launch), below one 16-byte group, around the wave (64) and the workgroup (256), several workgroups with a head and
a tail (4099) and more groups than one grid-stride round covers (2^20 + 7).  Every size sits 0..3 words past a 16-byte boundary
inside guard bands (tests/offset_buf.py); the kernel only reads, so the guards of the input and of the accumulator's buffer
must come back as they were."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import digest_ref as dr  # noqa: E402
import offset_buf as ob  # noqa: E402
from hp_vae_gan_amd import lib, ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SIZES = [0, 1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 4099, (1 << 20) + 7]
MASK = (1 << 64) - 1


def _words(n, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)


def _acc():
    """One int64 accumulator in the middle of a guarded buffer of int32 words (two words = the accumulator)."""
    view = ob.out_like((2,), torch.int32, 0, device=DEV)
    view.zero_()
    return view


def _acc_value(view):
    lo, hi = [int(v) & 0xFFFFFFFF for v in view.cpu().tolist()]
    return lo | (hi << 32)


def _raw(t, n, salt, acc):
    lib.call("hpvg_state_digest_u32", ctypes.c_void_p(t.data_ptr()) if t is not None else None, n, salt,
             ctypes.c_void_p(acc.data_ptr()), lib.stream())


@pytest.mark.parametrize("n", SIZES)
def test_digest_equals_the_reference_at_every_offset(n):
    w = _words(n, n)
    t = torch.from_numpy(w.view(np.int32).copy())
    for off in ob.OFFSETS:
        if n == 0:      # an empty view has no address of its own: the pointer of a one-word payload, and no word to read
            x = ob.embed(torch.zeros(1, dtype=torch.int32), off, guard=64, device=DEV)
            acc = _acc()
            _raw(x, 0, 7, acc)
            assert _acc_value(acc) == 0 and ob.guards_intact(x) and ob.guards_intact(acc) and int(x.item()) == 0
            assert ops.state_digest([x[:0]]) == 0 and ops.state_digest([x[:0], x]) == dr.digest([0])
            continue
        x = ob.embed(t, off, guard=64, device=DEV)
        assert ob.residue(x) == 4 * off
        salt = 0 if off < 2 else (1 << 40) + 3 * off
        acc = _acc()
        _raw(x, n, salt, acc)
        want = dr.digest(w, salt)
        assert _acc_value(acc) == want, (n, off)
        # accumulated over two calls
        _raw(x, n, salt + 1, acc)
        assert _acc_value(acc) == (want + dr.digest(w, salt + 1)) & MASK, (n, off)
        assert ob.guards_intact(x) and ob.guards_intact(acc), (n, off)
        assert np.array_equal(x.cpu().numpy().view(np.uint32), w)
        if off == 1:
            assert ops.state_digest([x]) == dr.digest(w)


def test_split_calls_equal_one_call_and_bad_arguments_are_refused():
    w = _words(1000, 7)
    t = torch.from_numpy(w.view(np.int32).copy()).to(DEV)
    whole = ops.state_digest([t])
    assert whole == dr.digest(w)
    assert ops.state_digest([t[:333], t[333:334], t[334:]]) == whole
    assert ops.state_digest([]) == 0
    acc = torch.zeros(1, dtype=torch.int64, device=DEV)
    for args in ((t, -1, 0, acc), (None, 4, 0, acc)):
        with pytest.raises(RuntimeError, match="HPVG_ERR_ARG"):
            _raw(*args)
    with pytest.raises(RuntimeError, match="HPVG_ERR_ARG"):
        lib.call("hpvg_state_digest_u32", ctypes.c_void_p(t.data_ptr()), 4, 0, None, lib.stream())
    _raw(None, 0, 0, acc)     # n == 0: nothing to read, OK
    assert int(acc.item()) == 0
    with pytest.raises(RuntimeError, match="4-byte and 8-byte"):
        ops.state_digest([torch.zeros(4, dtype=torch.uint8, device=DEV)])


def test_float_bit_patterns_int64_and_a_second_stream():
    f = np.array([0.0, -0.0, np.nan, -np.nan, np.inf, 1.5, 1e-45], dtype=np.float32)
    f = np.concatenate([f, np.array([0x7FC0BEEF, 0xFFFFFFFF], dtype=np.uint32).view(np.float32)])
    ft = torch.from_numpy(f.copy()).to(DEV)
    assert ops.state_digest([ft]) == dr.digest(dr.words_of(f))
    assert ops.state_digest([ft]) != ops.state_digest([torch.where(ft == 0, torch.zeros_like(ft), ft)])   # -0.0 is not 0.0
    i64 = np.array([0x1122334455667788, -2, 0, 1 << 40], dtype=np.int64)
    it = torch.from_numpy(i64.copy()).to(DEV)
    assert ops.state_digest([it]) == dr.digest(dr.words_of(i64))
    d = np.array([1.0, -0.0, np.nan], dtype=np.float64)
    assert ops.state_digest([torch.from_numpy(d.copy()).to(DEV)]) == dr.digest(dr.words_of(d))
    want = dr.digest_arrays([f, i64])
    assert ops.state_digest([ft, it]) == want
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert ops.state_digest([ft, it]) == want
    torch.cuda.current_stream().wait_stream(side)


def test_captured_launch_advances_acc_by_the_same_amount_each_replay():
    w = _words(5000, 11)
    t = torch.from_numpy(w.view(np.int32).copy()).to(DEV)[1:]     # one word past a 16-byte boundary
    acc = torch.zeros(1, dtype=torch.int64, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.state_digest_(t, 5, acc)
    torch.cuda.current_stream().wait_stream(side)
    one = dr.digest(w[1:], 5)
    assert int(acc.item()) & MASK == one
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.state_digest_(t, 5, acc)
    torch.cuda.synchronize()
    assert int(acc.item()) & MASK == one                          # recording executes nothing
    for k in (2, 3):
        graph.replay()
        torch.cuda.synchronize()
        assert int(acc.item()) & MASK == (k * one) & MASK, k
