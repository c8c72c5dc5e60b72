"""evaluate --prdc on the host: the yardstick (tests/prdc_ref.py) against answers worked by hand on 1-D point sets, seeded
defects that those answers reject, prdc_metrics, the flags' refusals and the values of the program tests' fixture.

The point sets are [1,1,W,3] volumes with patch 1 x 1 x 1 whose channel 0 holds the coordinate (channels 1 and 2 are 0), so
d2 is the squared difference of two coordinates and every figure below can be read off:

  R = 0 1 3 7 7 20 21 80     nearest other point at distance^2  1 1 4 0 0 1 1 3481   (the duplicate pair has radius 0)
  S = 2 7 11 40              nearest other point at distance^2  25 16 16 841

At k = 1, d2(s = 2, r = 1) = 1 equals r's radius: the `<=` of the definition decides it."""
import ctypes

import numpy as np
import pytest

from hp_vae_gan_amd import evaluate, ops
from hp_vae_gan_amd import lib as hplib

import prdc_ref
from prdc_ref import dist2, patches, ref_ball_count, ref_knn_self, ref_prdc

ONE = (1, 1, 1)
I3 = ctypes.c_int * 3
FOUR = ("precision", "recall", "density", "coverage")


def _points(xs):
    v = np.zeros((1, 1, len(xs), 3), np.uint8)
    v[0, 0, :, 0] = xs
    return v


R = _points([0, 1, 3, 7, 7, 20, 21, 80])
S = _points([2, 7, 11, 40])


# ------------------------------------------------------------------------------------------------------- by hand
def test_radii_by_hand():
    assert ref_knn_self(R, ONE, 1)[0, 0, :, 0].tolist() == [1, 1, 4, 0, 0, 1, 1, 3481]
    assert ref_knn_self(S, ONE, 1)[0, 0, :, 0].tolist() == [25, 16, 16, 841]
    # k = 2, all columns: ascending, the duplicate's 0 first, then the next point
    assert ref_knn_self(R, ONE, 2)[0, 0].tolist() == [[1, 9], [1, 4], [4, 9], [0, 16], [0, 16], [1, 169], [1, 196], [3481, 3600]]
    # three equal points: each has TWO others at distance 0 (multiplicity), the third neighbour is the far point
    assert ref_knn_self(_points([5, 5, 5, 9]), ONE, 3)[0, 0].tolist() == [[0, 0, 16], [0, 0, 16], [0, 0, 16], [16, 16, 16]]


def test_ball_count_by_hand():
    rad = [1, 1, 4, 0, 0, 1, 1, 3481]
    # s = 2: r = 1 (1 <= 1, equality) and r = 3; s = 7: the two 7s; s = 11: nobody; s = 40: only the wide ball of 80
    assert ref_ball_count(S, R, rad, ONE)[0, 0].tolist() == [2, 2, 0, 1]
    assert ref_ball_count(S, R, [0] * 8, ONE)[0, 0].tolist() == [0, 2, 0, 0]
    # the radius belongs to the KEY: the other way round the queries are R and the balls S's
    assert ref_ball_count(R, S, [25, 16, 16, 841], ONE)[0, 0].tolist() == [1, 1, 2, 3, 3, 1, 1, 0]   # r = 3: s = 2 and, at 16 <= 16, s = 7


HAND = {
    1: {"precision": 3 / 4, "density": 5 / 4, "recall": 7 / 8, "coverage": 5 / 8},
    2: {"precision": 4 / 4, "density": 12 / 8, "recall": 7 / 8, "coverage": 8 / 8},
}


@pytest.mark.parametrize("k", [1, 2])
def test_prdc_by_hand(k):
    w = ref_prdc(R, S, ONE, k)
    assert {n: w[n] for n in FOUR} == HAND[k]
    if k == 1:
        assert w["count"][0, 0].tolist() == [2, 2, 0, 1] and w["zero_radius"] == 2
        assert w["real_covered"][0, 0].tolist() == [False, True, True, True, True, False, False, True]


def test_floor_by_hand():
    # floor(X * D * 255^2) = 4 with D = 3: every radius below 4 becomes 4, on both sides; zero_radius counts the unfloored ones
    w = ref_prdc(R, S, ONE, 1, floor=4.5 / (3 * 255 * 255))
    assert w["real_radius"][0, 0].tolist() == [4, 4, 4, 4, 4, 4, 4, 3481] and w["zero_radius"] == 2
    assert w["count"][0, 0].tolist() == [3, 2, 0, 1]      # s = 2 now also lies in the ball of r = 0 (4 <= 4)
    assert {n: w[n] for n in FOUR} == {"precision": 3 / 4, "density": 6 / 4, "recall": 7 / 8, "coverage": 6 / 8}


# ------------------------------------------------------------------------------------------------ seeded defects
def _variant(real, smp, k, defect=None):
    """The yardstick restated with one switch per defect; without a defect it is ref_prdc."""
    Rm, _ = patches(real, ONE)
    Sm, _ = patches(smp, ONE)
    Nr, Ns = len(Rm), len(Sm)

    def radius(X):
        d = dist2(X, X)
        if defect != "self":
            d[np.arange(len(X)), np.arange(len(X))] = np.iinfo(np.int64).max
        return np.sort(d, axis=1)[:, max(k - 2, 0) if defect == "k-1" else k - 1]

    rad_R, rad_S = radius(Rm), radius(Sm)
    d = dist2(Sm, Rm)
    le = (lambda a, b: a < b) if defect == "strict" else (lambda a, b: a <= b)
    if defect == "query radius":
        inside, reached = le(d, rad_S[:, None]), le(d, rad_R[None, :]).any(0)
    else:
        inside, reached = le(d, rad_R[None, :]), le(d, rad_S[:, None]).any(0)
    count = inside.sum(1)
    covered = le(d.min(0), rad_R)
    return {"precision": int((count > 0).sum()) / Ns, "density": int(count.sum()) / ((1 if defect == "no k" else k) * Ns),
            "recall": int(reached.sum()) / Nr, "coverage": int(covered.sum()) / Nr}


def test_the_variant_without_a_defect_is_the_yardstick():
    for k in (1, 2):
        assert _variant(R, S, k) == HAND[k]


@pytest.mark.parametrize("defect", ["self", "k-1", "strict", "query radius", "no k"])
def test_seeded_defects_change_a_hand_worked_answer(defect):
    assert any(_variant(R, S, k, defect) != HAND[k] for k in (1, 2)), defect


# ------------------------------------------------------------------------------------------------- prdc_metrics
def test_prdc_metrics_on_integer_counts():
    m = evaluate.prdc_metrics(0, 0, 0, 0, 1188, 1188, 3)
    assert m == {"precision": 0.0, "recall": 0.0, "density": 0.0, "coverage": 0.0}
    assert all(type(v) is float for v in m.values())
    m = evaluate.prdc_metrics(1188, 3 * 1188, 700, 700, 1188, 700, 3)
    assert m == {"precision": 1.0, "recall": 1.0, "density": 1.0, "coverage": 1.0}
    assert evaluate.prdc_metrics(3, 5, 7, 5, 4, 8, 1) == HAND[1]
    # density is not bounded by 1: a copy lies in its own ball and in its k neighbours'
    assert evaluate.prdc_metrics(10, 40, 10, 10, 10, 10, 3)["density"] == 4 / 3
    # counts past 2^31 stay exact (Python ints)
    assert evaluate.prdc_metrics(1, 3 * 2 ** 40, 1, 1, 2 ** 40, 1, 3)["density"] == 1.0


# -------------------------------------------------------------------------------------------------------- flags
def test_parser_flags():
    p = evaluate.evaluate_parser()
    a = p.parse_args(["--exp-dir", "e"])
    assert (a.prdc, a.prdc_floor, a.save_prdc) == (0, None, False)
    a = p.parse_args(["--exp-dir", "e", "--prdc", "3", "--prdc-floor", "0.01", "--save-prdc"])
    assert (a.prdc, a.prdc_floor, a.save_prdc) == (3, 0.01, True)
    assert p.parse_args(["--exp-dir", "e", "--prdc", "8"]).prdc == 8
    for bad in (["--prdc", "9"], ["--prdc", "-1"], ["--prdc", "x"], ["--prdc-floor", "-0.5"], ["--prdc-floor", "nan"]):
        with pytest.raises(SystemExit):
            p.parse_args(["--exp-dir", "e"] + bad)


def test_floor_without_prdc_and_k_out_of_range_end_the_program_before_any_device_work(tmp_path):
    np.save(str(tmp_path / "S.npy"), np.zeros((1, 3, 8, 8, 3), np.uint8))
    np.save(str(tmp_path / "R.npy"), np.zeros((3, 8, 8, 3), np.uint8))
    files = dict(samples=str(tmp_path / "S.npy"), real=str(tmp_path / "R.npy"))
    with pytest.raises(SystemExit, match="--prdc-floor needs --prdc"):
        evaluate.evaluate(prdc_floor=0.1, **files)
    with pytest.raises(SystemExit, match="--prdc-floor needs --prdc"):
        evaluate.main(["--samples", files["samples"], "--real", files["real"], "--prdc-floor", "0.1"])
    for k in (9, -1):
        with pytest.raises(SystemExit, match=r"--prdc K must be in \[1, 8\], got %d" % k):
            evaluate.evaluate(prdc=k, **files)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["R.npy", "S.npy"]


def test_too_few_patches_names_the_count_and_k():
    evaluate.prdc_check(0)
    evaluate.prdc_check(3, None, 4, 4)
    evaluate.prdc_check(3, 0.0, 4, 1188)
    with pytest.raises(SystemExit, match="sample has 3 patches.*k = 3"):
        evaluate.prdc_check(3, None, 3, 1188)
    with pytest.raises(SystemExit, match="real volume has 2 patches.*k = 3"):
        evaluate.prdc_check(3, None, 1188, 2)
    with pytest.raises(SystemExit, match="must be a finite number >= 0"):
        evaluate.prdc_check(3, -1.0)


def test_the_c_entries_refuse_bad_k_and_small_sets_on_the_host():
    lib = hplib.load()
    one, patch = I3(1, 1, 1), I3(3, 7, 7)
    assert lib.hpvg_patchknn_self_ws_bytes(4, 20, 23, patch, one, 3) > 0
    dummy = ctypes.create_string_buffer(64)
    p = ctypes.cast(dummy, ctypes.c_void_p)
    for shape, pa, st, k in [((4, 20, 23), patch, one, 0), ((4, 20, 23), patch, one, 9), ((4, 20, 23), patch, one, -1),
                             ((3, 7, 10), patch, one, 4), ((3, 7, 10), patch, one, 5),      # N = 4 <= k
                             ((2, 20, 23), patch, one, 1), ((4, 20, 23), patch, I3(1, 0, 1), 1)]:
        assert lib.hpvg_patchknn_self_ws_bytes(*shape, pa, st, k) == 0
        # the launch entry refuses before it touches a pointer or the device
        assert lib.hpvg_patchknn_self_u8(p, *shape, pa, st, k, p, p, 64, None) == -1
    assert lib.hpvg_patchknn_self_ws_bytes(3, 7, 10, patch, one, 3) > 0                        # N = k + 1
    assert lib.hpvg_patch_ball_count_ws_bytes(4, 20, 23, 5, 17, 31, patch, one, one) > 0
    assert lib.hpvg_patch_ball_count_ws_bytes(2, 20, 23, 5, 17, 31, patch, one, one) == 0
    assert lib.hpvg_patch_ball_count_u8(p, 2, 20, 23, p, 5, 17, 31, patch, one, one, p, p, p, 64, None) == -1
    assert lib.hpvg_patch_ball_count_u8(p, 4, 20, 23, p, 5, 17, 31, patch, one, one, None, p, p, 64, None) == -1
    assert ops.PATCH_KNN_MAX_K == 8


# ------------------------------------------------------------------------------------------ the program fixture
def test_the_program_fixture_has_a_sample_no_constant_could_pass():
    real, smp = prdc_ref.program_fixture()
    assert real.shape == (5, 24, 28, 3) and smp.shape == (3, 5, 24, 28, 3) and np.array_equal(smp[0], real)
    copy, half, noisy = prdc_ref.program_want(3)
    assert (copy["precision"], copy["recall"], copy["coverage"], copy["density"]) == (1.0, 1.0, 1.0, 4 / 3)
    # the right half repeats the left: every patch is still (nearly) a real patch, yet under half of the real ones are reached
    assert all(0.1 < half[n] < 0.99 for n in FOUR), half
    assert half["precision"] > 0.7 and half["recall"] < 0.5 and half["coverage"] < 0.5 and half["density"] > 0.9
    assert len({(w["precision"], w["recall"], w["density"], w["coverage"]) for w in (copy, half, noisy)}) == 3
