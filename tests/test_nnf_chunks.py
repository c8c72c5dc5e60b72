"""The yardstick of the chunk labelling (tests/nnf_chunks_ref.py) against answers worked out by hand, the arithmetic of
evaluate.chunk_metrics, evaluate's new flags, and the refusals of hpvg_nnf_chunks_i32, which touch no device.  No GPU."""
import ctypes

import numpy as np
import pytest

from hp_vae_gan_amd import evaluate
from hp_vae_gan_amd import lib as hplib

from nnf_chunks_ref import pair_count, ref_chunks, same

ERR_ARG = -1
I3 = ctypes.c_int * 3


# ------------------------------------------------------------------------------------------------------------ yardstick
def test_one_patch_grid():
    labels, sizes, stats = ref_chunks(np.array([[[0]]], np.int32), (1, 1, 1))
    assert labels.tolist() == [[[0]]] and sizes.tolist() == [[[1]]]
    assert stats.tolist() == [1, 1, 0, 1, 1, 1]   # kept, in place, no pair at all, one chunk of one patch
    assert pair_count((1, 1, 1)) == 0
    labels, sizes, stats = ref_chunks(np.array([[[-1]]], np.int32), (1, 1, 1))
    assert labels.tolist() == [[[-1]]] and sizes.tolist() == [[[0]]] and stats.tolist() == [0, 0, 0, 0, 0, 0]


def test_a_1x2x3_grid_by_hand():
    # key grid (1, 3, 5).  Query coordinate -> key coordinate -> displacement (y, x):
    #   (0,0) -> 6 = (1,1): (1,1)    (0,1) -> 7 = (1,2): (1,1)    (0,2) -> 2 = (0,2): (0,0)
    #   (1,0) -> 11 = (2,1): (1,1)   (1,1) -> 6 = (1,1): (0,0)    (1,2) -> 7 = (1,2): (0,0)
    # coherent pairs: 0-1 (x), 0-3 (y), 4-5 (x); 2-5 is a pair (y) with (0,0) on both sides -> coherent too.
    nn = np.array([[[6, 7, 2], [11, 6, 7]]], np.int32)
    labels, sizes, stats = ref_chunks(nn, (1, 3, 5))
    assert labels.tolist() == [[[0, 0, 2], [0, 2, 2]]]
    assert sizes.tolist() == [[[3, 0, 3], [0, 0, 0]]]
    assert pair_count((1, 2, 3)) == 7
    assert stats.tolist() == [6, 3, 4, 2, 3, 18]
    # the 2-D form is the same grid
    l2, s2, st2 = ref_chunks(nn[0], (1, 3, 5))
    assert l2.tolist() == labels[0].tolist() and s2.tolist() == sizes[0].tolist() and st2.tolist() == stats.tolist()
    # a threshold on d2 takes patch 0 out: 1 and 3 lose their link
    d2 = np.array([[[9, 0, 0], [0, 0, 0]]], np.int32)
    labels, sizes, stats = ref_chunks(nn, (1, 3, 5), d2=d2, max_d2=8)
    assert labels.tolist() == [[[-1, 1, 2], [3, 2, 2]]]
    assert sizes.tolist() == [[[0, 1, 3], [1, 0, 0]]]
    assert stats.tolist() == [5, 3, 2, 3, 3, 11]
    # strides: with qstride (1, 1, 2) the x displacement of (0,0), (0,1) is 1 - 0 = 1 and 2 - 2 = 0: that pair falls apart
    labels, _, stats = ref_chunks(nn, (1, 3, 5), qstride=(1, 1, 2))
    assert labels[0, 0].tolist()[:2] == [0, 1]


def test_seeded_defects_are_rejected():
    # grid (2, 3, 4): the outer columns carry one displacement, the inner ones others, so a row-end link merges columns
    g = (2, 3, 4)
    kW = 8
    t, y, x = np.meshgrid(*(np.arange(n) for n in g), indexing="ij")
    dx = np.where((x == 0) | (x == g[2] - 1), 0, x)
    nn = ((t * 3 + y) * kW + x + dx).astype(np.int32)
    want = ref_chunks(nn, (2, 3, kW))
    assert want[2].tolist()[3] == 4 and same(want, ref_chunks(nn, (2, 3, kW)))
    off = want[0].copy()
    off[1, 2, 3] = 0
    assert not same((off, want[1], want[2]), want)
    size = want[1].copy()
    size[0, 1, 0] = 6   # a non-root
    assert want[0][0, 1, 0] != 4 and not same((want[0], size, want[2]), want)
    wrapped = ref_chunks(nn, (2, 3, kW), wrap_defect=True)
    assert wrapped[2].tolist()[3] == 3 and not same(wrapped, want)


# ------------------------------------------------------------------------------------------------------------ evaluate, host side
def test_chunk_metrics_by_hand():
    m = evaluate.chunk_metrics([6, 3, 4, 2, 3, 18], 6, 7)
    assert m == {"nnf_coherence": 4 / 7, "chunks": 2, "largest_chunk_frac": 0.5, "chunk_frac": 0.5, "in_place_frac": 0.5}
    m = evaluate.chunk_metrics(np.array([864, 0, 2148, 2, 432, 373248], np.int64), 1188, 3048, kept_frac=True)
    assert m == {"nnf_coherence": 2148 / 3048, "chunks": 2, "largest_chunk_frac": 432 / 1188, "chunk_frac": 373248 / 1411344,
                 "in_place_frac": 0.0, "chunk_kept_frac": 864 / 1188}
    assert evaluate.chunk_metrics([1, 1, 0, 1, 1, 1], 1, 0)["nnf_coherence"] is None
    assert evaluate.chunk_metrics([1188, 1188, 3048, 1, 1188, 1188 * 1188], 1188, 3048) == \
        {"nnf_coherence": 1.0, "chunks": 1, "largest_chunk_frac": 1.0, "chunk_frac": 1.0, "in_place_frac": 1.0}
    # integers past 2^53 still divide exactly (int / int is correctly rounded)
    big = 2 ** 31 - 1
    assert evaluate.chunk_metrics([big, 0, 0, 1, big, big * big], big, 1)["chunk_frac"] == 1.0
    assert evaluate.pair_count((3, 18, 22)) == 3048 == pair_count((3, 18, 22)) and evaluate.pair_count((1, 1, 1)) == 0


def test_parser_flags():
    p = evaluate.evaluate_parser()
    a = p.parse_args(["--exp-dir", "e"])
    assert (a.chunks, a.chunk_tol, a.save_chunks) == (False, None, False)
    a = p.parse_args(["--exp-dir", "e", "--chunks", "--chunk-tol", "0.25", "--save-chunks"])
    assert (a.chunks, a.chunk_tol, a.save_chunks) == (True, 0.25, True)
    assert p.parse_args(["--exp-dir", "e", "--chunk-tol", "0"]).chunk_tol == 0.0
    for bad in ("-0.5", "nan", "inf", "x"):
        with pytest.raises(SystemExit):
            p.parse_args(["--exp-dir", "e", "--chunk-tol", bad])


def test_source_colours():
    import torch
    nn = torch.tensor([[[0, 4], [14, 29]]], dtype=torch.int32)   # key grid (2, 3, 5): (0,0,0) (0,0,4) (0,2,4) (1,2,4)
    c = evaluate.source_colours(nn, (2, 3, 5))
    assert c.dtype == torch.uint8 and c.tolist() == [[[[0, 0, 0], [255, 0, 0]], [[255, 255, 0], [255, 255, 255]]]]
    c = evaluate.source_colours(torch.tensor([[1, 2]], dtype=torch.int32), (1, 1, 5))   # x = 1, 2 of 5: 63.75 -> 64, 127.5 -> 128
    assert c.tolist() == [[[64, 0, 0], [128, 0, 0]]]


# ------------------------------------------------------------------------------------------------------------ refusals
BAD = {
    "null nn": dict(nn=None),
    "null labels": dict(labels=None),
    "null sizes": dict(sizes=None),
    "null stats": dict(stats=None),
    "query grid entry 0": dict(qgrid=(2, 0, 4)),
    "key grid entry -1": dict(rgrid=(2, 3, -1)),
    "query stride 0": dict(qstride=(1, 0, 1)),
    "key stride -2": dict(rstride=(-2, 1, 1)),
    "Nq = 2^31": dict(qgrid=(2048, 1024, 1024)),
    "Nr = 2^31": dict(rgrid=(2048, 1024, 1024)),
    "negative max_d2 with d2": dict(d2=True, max_d2=-1),
}


@pytest.mark.parametrize("why", sorted(BAD))
def test_bad_arguments_return_err_arg(why):
    lib = hplib.load()
    dummy = ctypes.create_string_buffer(64)
    p = ctypes.cast(dummy, ctypes.c_void_p)
    a = dict(nn=p, d2=None, max_d2=0, qgrid=(2, 3, 4), rgrid=(2, 3, 4), qstride=(1, 1, 1), rstride=(1, 1, 1), labels=p, sizes=p, stats=p)
    a.update(BAD[why])
    if a["d2"] is True:
        a["d2"] = p
    # the entry point refuses before it touches a pointer or the device
    assert lib.hpvg_nnf_chunks_i32(a["nn"], a["d2"], a["max_d2"], I3(*a["qgrid"]), I3(*a["rgrid"]), I3(*a["qstride"]),
                                   I3(*a["rstride"]), a["labels"], a["sizes"], a["stats"], None) == ERR_ARG


def test_null_geometry_arrays_are_refused_and_the_symbol_is_bound():
    lib = hplib.load()
    p = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)
    one = I3(1, 1, 1)
    for k in range(4):
        geo = [one, one, one, one]
        geo[k] = None
        assert lib.hpvg_nnf_chunks_i32(p, None, 0, *geo, p, p, p, None) == ERR_ARG
    assert "hpvg_nnf_chunks_i32" in hplib.check_symbols()
