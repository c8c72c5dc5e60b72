"""evaluate --prdc on the GPU against the yardstick of tests/prdc_ref.py, on its program fixture: a smooth 5 x 24 x 28 volume
and three samples - the copy, the volume whose right half repeats its left half, a noisy copy.  Every figure is compared with
==: the program's integers are exact and each score is one Python int / int division on both sides.
(tests/test_prdc.py asserts that the half-duplicated sample's four values lie strictly inside (0.1, 0.99).)"""
import json

import numpy as np
import pytest

from hp_vae_gan_amd import evaluate

import prdc_ref
from test_evaluate_gpu import KEYS

pytestmark = pytest.mark.gpu
FOUR = ("precision", "recall", "density", "coverage")
PER_SAMPLE = {"coherence", "completeness", "nn_unique_frac"}
TOP = set(FOUR) | {"prdc_k", "prdc_floor", "prdc_zero_radius_frac", "prdc_seconds"}


def _files(tmp_path, real, samples):
    np.save(str(tmp_path / "S.npy"), samples)
    np.save(str(tmp_path / "R.npy"), real)
    return dict(samples=str(tmp_path / "S.npy"), real=str(tmp_path / "R.npy"))


def _run(tmp_path, capsys, real=None, samples=None, **kw):
    if real is None:
        real, samples = prdc_ref.program_fixture()
    m = evaluate.evaluate(**_files(tmp_path, real, samples), **kw)
    line = capsys.readouterr().out.strip().splitlines()
    with open(str(tmp_path / "metrics.json")) as f:
        assert json.load(f) == m
    return m, line


def _same_as(m, want, k=3, floor=None):
    assert set(m) == KEYS | TOP and all(set(p) == PER_SAMPLE | set(FOUR) for p in m["per_sample"])
    assert len(m["per_sample"]) == len(want)
    for p, w in zip(m["per_sample"], want):
        assert {n: p[n] for n in FOUR} == {n: w[n] for n in FOUR}
    for n in FOUR:
        assert m[n] == sum(w[n] for w in want) / len(want)
    Nr = want[0]["real_radius"].size
    assert (m["prdc_k"], m["prdc_floor"], m["prdc_zero_radius_frac"]) == (k, floor, want[0]["zero_radius"] / Nr)
    assert m["prdc_seconds"] > 0


def test_prdc_equals_the_yardstick_and_saves_its_arrays(tmp_path, capsys):
    real, samples = prdc_ref.program_fixture()
    files = _files(tmp_path, real, samples)
    assert evaluate.main(["--samples", files["samples"], "--real", files["real"], "--prdc", "3", "--save-prdc"]) == 0
    line = capsys.readouterr().out.strip().splitlines()
    with open(str(tmp_path / "metrics.json")) as f:
        m = json.load(f)
    want = prdc_ref.program_want(3)
    _same_as(m, want)
    copy, half = m["per_sample"][0], m["per_sample"][1]
    assert (copy["precision"], copy["recall"], copy["coverage"]) == (1.0, 1.0, 1.0) and copy["density"] == 4 / 3
    assert all(0.1 < half[n] < 0.99 for n in FOUR)
    assert len(line) == 1 and " precision {:.6f} recall {:.6f} density {:.6f} coverage {:.6f} (".format(
        *(m[n] for n in FOUR)) in line[0]
    z = np.load(str(tmp_path / "prdc.npz"))
    assert set(z.files) == {"count", "real_radius", "real_covered"}
    assert z["count"].dtype == np.int32 and z["count"].shape == (3, 3, 18, 22)
    assert z["real_radius"].shape == (3, 18, 22) and z["real_covered"].shape == (3, 3, 18, 22)
    assert np.array_equal(z["real_radius"], want[0]["real_radius"])
    for i, w in enumerate(want):
        assert np.array_equal(z["count"][i], w["count"]) and np.array_equal(z["real_covered"][i], w["real_covered"])


def test_prdc_on_the_strided_sample_grid(tmp_path, capsys):
    m, _ = _run(tmp_path, capsys, prdc=3, stride=(1, 2, 3))
    want = prdc_ref.program_want(3, (1, 2, 3))
    assert (m["Nq"], m["Nr"]) == (3 * 9 * 8, 3 * 18 * 22) and want[0]["count"].shape == (3, 9, 8)
    _same_as(m, want)
    assert m["per_sample"][0]["coverage"] < 1.0     # a third of the copy's patches do not reach every real patch


def test_prdc_floor_raises_the_radii(tmp_path, capsys):
    m, _ = _run(tmp_path, capsys, prdc=3, prdc_floor=1e-3, save_prdc=True)
    want, plain = prdc_ref.program_want(3, (1, 1, 1), 1e-3), prdc_ref.program_want(3)
    assert int(np.floor(1e-3 * 441 * 255 * 255)) == 28676 and int(want[0]["real_radius"].min()) == 28676
    assert int(plain[0]["real_radius"].min()) < 28676 < int(plain[0]["real_radius"].max())
    assert all(w["density"] > p["density"] for w, p in zip(want, plain))
    _same_as(m, want, floor=1e-3)
    assert np.array_equal(np.load(str(tmp_path / "prdc.npz"))["real_radius"], want[0]["real_radius"])


def test_prdc_other_k(tmp_path, capsys):
    m, _ = _run(tmp_path, capsys, prdc=5)
    _same_as(m, prdc_ref.program_want(5), k=5)


def test_prdc_on_images(tmp_path, capsys):
    real, samples = prdc_ref.program_fixture()
    real, samples = np.ascontiguousarray(real[2]), np.ascontiguousarray(samples[:, 2])
    m, _ = _run(tmp_path, capsys, real, samples, prdc=3, save_prdc=True)
    want = [prdc_ref.ref_prdc(real, s, (1, 7, 7), 3) for s in samples]
    assert m["patch"] == [1, 7, 7] and m["Nq"] == 18 * 22
    _same_as(m, want)
    z = np.load(str(tmp_path / "prdc.npz"))
    assert z["count"].shape == (3, 1, 18, 22) and np.array_equal(z["count"], np.stack([w["count"] for w in want]))


def test_without_the_flag_nothing_changes(tmp_path, capsys):
    m, line = _run(tmp_path, capsys, save_prdc=True)     # --save-prdc implies nothing on its own
    assert set(m) == KEYS and all(set(p) == PER_SAMPLE for p in m["per_sample"])
    assert len(line) == 1 and not any(w in line[0] for w in ("precision", "recall", "density", "coverage"))
    assert sorted(p.name for p in tmp_path.iterdir()) == ["R.npy", "S.npy", "metrics.json"]
    with_prdc, _ = _run(tmp_path, capsys, prdc=3)
    for key in KEYS - {"patchnn_seconds", "per_sample"}:
        assert with_prdc[key] == m[key], key
    for a, b in zip(with_prdc["per_sample"], m["per_sample"]):
        assert {n: a[n] for n in PER_SAMPLE} == b
