"""hpvg_volume_resize_u8 (ops.volume_resize_u8) on the GPU against the numpy restatement of the contract (tests/volresize_ref.py).
Everything is exact: every byte.  The shapes cover both shapes of the kernel (a thread per output voxel; a wave per output
voxel from 64 source voxels per output on), every kind of axis (down, up, equal, to one, from one), more than one workgroup,
and the row whose sum passes 2^31."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from hp_vae_gan_amd import lib as hplib  # noqa: E402
from hp_vae_gan_amd import ops  # noqa: E402
import offset_buf as OB  # noqa: E402
import volresize_ref as VR  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [((5, 9, 11), (3, 4, 5)), ((3, 4, 5), (5, 9, 11)), ((4, 7, 6), (4, 3, 13)), ((5, 9, 11), (1, 1, 1)), ((2, 3, 2), (1, 5, 1)),
          ((1, 1, 1), (2, 3, 4)), ((1, 8, 8), (1, 3, 5)), ((1, 64, 64), (1, 3, 3)), ((9, 33, 2), (2, 2, 2)), ((7, 40, 48), (5, 30, 36)),
          ((1, 1, 4096), (1, 1, 1))]
KINDS = ("bytes", "binary", "white")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _case(src, out, kind):
    """(volume, the reference's bytes) - built once, shared, never modified."""
    rng = np.random.default_rng(hash((src, out)) % 1000 + KINDS.index(kind))
    if kind == "bytes":
        v = rng.integers(0, 256, size=src + (3,), dtype=np.uint8)
    elif kind == "binary":
        v = (rng.integers(0, 2, size=src + (3,), dtype=np.uint8) * 255).astype(np.uint8)
    else:
        v = np.full(src + (3,), 255, np.uint8)
    return v, VR.resize(v, out)


@pytest.mark.parametrize("kind", KINDS[:2])
@pytest.mark.parametrize("src,out", SHAPES, ids=["%dx%dx%d-%dx%dx%d" % (s + o) for s, o in SHAPES])
def test_equals_the_reference(src, out, kind):
    v, want = _case(src, out, kind)
    got = ops.volume_resize_u8(_dev(v), out)
    assert got.dtype == torch.uint8 and tuple(got.shape) == out + (3,) and got.is_contiguous()
    assert np.array_equal(got.cpu().numpy(), want)


def test_both_kernel_shapes_and_the_threshold_between_them():
    reads = [VR.dmax_and_reads(s, o)[1] for s, o in SHAPES]
    assert min(reads) < 64 <= max(reads)
    assert any(o[0] * o[1] * o[2] > 256 for s, o in SHAPES if VR.dmax_and_reads(s, o)[1] < 64)        # more than one workgroup
    assert any(o[0] * o[1] * o[2] > 4 for s, o in SHAPES if VR.dmax_and_reads(s, o)[1] >= 64)
    # 63 source voxels per output: the last thread-per-output case; 64: the first wave-per-output one
    for src, out, n in (((1, 3, 63), (1, 3, 1), 63), ((1, 3, 64), (1, 3, 1), 64), ((3, 3, 7), (1, 1, 1), 63), ((4, 4, 4), (1, 1, 1), 64)):
        assert VR.dmax_and_reads(src, out)[1] == n
        v, want = _case(src, out, "bytes")
        assert np.array_equal(ops.volume_resize_u8(_dev(v), out).cpu().numpy(), want), (src, out)


def test_a_row_whose_sum_passes_2_to_31():
    src, out = (1, 1, 4096), (1, 1, 1)
    v, want = _case(src, out, "white")
    assert 255 * VR.dmax_and_reads(src, out)[0] > 2 ** 31 and (want == 255).all()
    assert np.array_equal(ops.volume_resize_u8(_dev(v), out).cpu().numpy(), want)


def test_the_tie_rounds_up():
    v = np.array([0, 255], np.uint8).reshape(1, 1, 2, 1).repeat(3, 3)
    got = ops.volume_resize_u8(_dev(v), (1, 1, 3)).cpu().numpy()
    assert got[0, 0, :, 0].tolist() == [0, 128, 255] and np.array_equal(got, VR.resize(v, (1, 1, 3)))


def test_images_and_equal_sizes():
    v, _ = _case((1, 8, 8), (1, 3, 5), "bytes")
    img = _dev(v[0])
    for size in ((3, 5), (1, 3, 5)):
        got = ops.volume_resize_u8(img, size)
        assert tuple(got.shape) == (3, 5, 3) and np.array_equal(got.cpu().numpy(), VR.resize(v, (1, 3, 5))[0])
    same = ops.volume_resize_u8(img, (8, 8))
    assert torch.equal(same, img) and same.data_ptr() != img.data_ptr() and same.is_contiguous()
    with pytest.raises(RuntimeError, match="size must be"):
        ops.volume_resize_u8(img, (2, 3, 5))
    # a view that is not contiguous is taken by value
    big = _dev(np.random.default_rng(9).integers(0, 256, size=(4, 7, 12, 3), dtype=np.uint8))
    view = big[:, :, ::2]
    assert np.array_equal(ops.volume_resize_u8(view, (4, 3, 13)).cpu().numpy(), VR.resize(view.cpu().numpy(), (4, 3, 13)))


@pytest.mark.parametrize("src,out", [((5, 9, 11), (3, 4, 5)), ((1, 64, 64), (1, 3, 3))], ids=["thread", "wave"])
def test_odd_byte_offsets_inside_guard_bands(src, out):
    """Source and output each start at an odd byte inside an int32 payload between guard bands (tests/offset_buf.py): the
    launch writes its bytes and nothing else."""
    v, want = _case(src, out, "bytes")

    def inside(nbytes, odd, data=None):
        words = (nbytes + odd + 3) // 4 + 1
        if data is None:
            payload = OB.out_like((words,), torch.int32, 1, device="cuda")
        else:
            payload = OB.embed(torch.full((words,), -1, dtype=torch.int32, device="cuda"), 1)
        view = payload.view(torch.uint8)[odd:odd + nbytes]
        if data is not None:
            view.copy_(_dev(data).reshape(-1))
        assert view.data_ptr() % 2 == 1 and view.is_contiguous()
        return payload, view
    _, s = inside(v.size, 3, v)
    payload, o = inside(want.size, 5)
    before = payload.view(torch.uint8).clone()
    hplib.call("hpvg_volume_resize_u8", hplib.ptr(s), *src, hplib.ptr(o), *out, hplib.stream())
    torch.cuda.synchronize()
    assert np.array_equal(o.cpu().numpy().reshape(want.shape), want)
    after = payload.view(torch.uint8)
    assert OB.guards_intact(payload) and torch.equal(after[:5], before[:5]) and torch.equal(after[5 + o.numel():], before[5 + o.numel():])


def test_two_streams_give_equal_results():
    v, want = _case((7, 40, 48), (5, 30, 36), "bytes")
    w, want_w = _case((1, 64, 64), (1, 3, 3), "bytes")
    dv, dw = _dev(v), _dev(w)
    torch.cuda.synchronize()
    got = []
    for _ in range(2):
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            got.append((ops.volume_resize_u8(dv, (5, 30, 36)), ops.volume_resize_u8(dw, (1, 3, 3))))
    torch.cuda.synchronize()
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])
    assert np.array_equal(got[0][0].cpu().numpy(), want) and np.array_equal(got[0][1].cpu().numpy(), want_w)


def test_overlap_is_refused_and_nothing_is_written():
    buf = _dev(np.random.default_rng(4).integers(0, 256, size=4 * 6 * 6 * 3 + 64, dtype=np.uint8))
    before = buf.clone()
    n_src, n_out = 4 * 6 * 6 * 3, 2 * 3 * 3 * 3
    lib = hplib.load()
    for off in (0, 7, n_src - 1):                 # out starts inside src
        rc = lib.hpvg_volume_resize_u8(ctypes.c_void_p(buf.data_ptr()), 4, 6, 6, ctypes.c_void_p(buf.data_ptr() + off), 2, 3, 3, hplib.stream())
        assert rc == -1, off
    rc = lib.hpvg_volume_resize_u8(ctypes.c_void_p(buf.data_ptr() + 10), 4, 6, 6, ctypes.c_void_p(buf.data_ptr()), 2, 3, 3, hplib.stream())
    assert rc == -1                               # out ends inside src
    torch.cuda.synchronize()
    assert torch.equal(buf, before)
    # back to back is fine
    rc = lib.hpvg_volume_resize_u8(ctypes.c_void_p(buf.data_ptr()), 4, 6, 6, ctypes.c_void_p(buf.data_ptr() + n_src), 2, 3, 3, hplib.stream())
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(buf[:n_src], before[:n_src])
    want = VR.resize(before[:n_src].cpu().numpy().reshape(4, 6, 6, 3), (2, 3, 3))
    assert np.array_equal(buf[n_src:n_src + n_out].cpu().numpy().reshape(2, 3, 3, 3), want)
