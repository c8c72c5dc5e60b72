"""`generate_patchnn --wrap` on the GPU: patchnn_refine steps on a ring against the numpy composition (tests/patchwrap_ref.py) for
both searches, the roll-equivariance a ring gives the exact step, and the programs - generate_patchnn as fresh child processes
under their own timeout, evaluate in this process: equal bytes on a second run, the json, `evaluate --wrap` against the numpy
seam restatement, and the seam of the ring samples against the seam of the same seeds without the flag."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from hp_vae_gan_amd import evaluate, generate_patchnn  # noqa: E402
from patchwrap_ref import refine_wrap_ref, seam_ref  # noqa: E402
from test_patchnn import _rand  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
SHAPE = (6, 40, 56)
FLAGS = {"t": (1, 0, 0), "hw": (0, 1, 1), "thw": (1, 1, 1)}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------------------ refine steps
@pytest.mark.parametrize("alpha", [0.005, float("inf")])
@pytest.mark.parametrize("search", ["exact", "patchmatch"])
@pytest.mark.parametrize("axes", ["t", "thw"])
def test_refine_steps_equal_the_numpy_composition(axes, search, alpha):
    """Two steps: the second starts its PatchMatch searches from the first step's fields, which live on the periodic grids."""
    query, keys, values, patch, wrap = _rand((6, 16, 20), 1), _rand((5, 15, 22), 2), _rand((5, 15, 22), 3), (3, 7, 7), FLAGS[axes]
    alpha_abs = alpha * 441 * 255 * 255
    want1, fwd, rev, seed = refine_wrap_ref(query, keys, values, patch, alpha_abs, wrap, search, 2, 0)
    want2 = refine_wrap_ref(want1, keys, values, patch, alpha_abs, wrap, search, 2, seed, fwd, rev)[0]
    state = generate_patchnn.patchnn_search_state(seed=0, index=0)
    kw = dict(search=search, pm_iters=2, state=state, wrap=wrap)
    got1 = generate_patchnn.patchnn_refine(_dev(query), _dev(keys), _dev(values), patch, alpha_abs, **kw)
    assert got1.dtype == torch.uint8 and got1.shape == (6, 16, 20, 3) and np.array_equal(got1.cpu().numpy(), want1)
    grid = tuple(s if w else s - p + 1 for s, p, w in zip((6, 16, 20), patch, wrap))
    assert tuple(state["fwd"].shape) == grid and np.array_equal(state["fwd"].cpu().numpy(), fwd)
    assert (state["rev"] is None) == np.isinf(alpha) and (rev is None or np.array_equal(state["rev"].cpu().numpy(), rev))
    got2, score = generate_patchnn.patchnn_refine(got1, _dev(keys), _dev(values), patch, alpha_abs, return_score=True, **kw)
    assert np.array_equal(got2.cpu().numpy(), want2) and np.isfinite(score) and score >= 0
    plain = generate_patchnn.patchnn_refine(_dev(query), _dev(keys), _dev(values), patch, alpha_abs, search=search, pm_iters=2)
    assert not torch.equal(plain, got1)
    none = generate_patchnn.patchnn_refine(_dev(query), _dev(keys), _dev(values), patch, alpha_abs, search=search, pm_iters=2,
                                           wrap=(0, 0, 0))
    assert torch.equal(none, plain)


@pytest.mark.parametrize("axes", ["t", "hw", "thw"])
def test_the_exact_step_on_a_ring_commutes_with_a_roll(axes):
    wrap, patch = FLAGS[axes], (3, 7, 7)
    q, real = _dev(_rand((6, 16, 20), 4)), _dev(_rand((5, 15, 22), 5))
    shift = tuple(s * w for s, w in zip((2, 5, 7), wrap))
    alpha_abs = 0.005 * 441 * 255 * 255
    step = lambda v, w: generate_patchnn.patchnn_refine(v, real, real, patch, alpha_abs, wrap=w)   # noqa: E731
    assert torch.equal(step(torch.roll(q, shift, (0, 1, 2)).contiguous(), wrap), torch.roll(step(q, wrap), shift, (0, 1, 2)))
    assert not torch.equal(step(torch.roll(q, shift, (0, 1, 2)).contiguous(), None), torch.roll(step(q, None), shift, (0, 1, 2)))


# ----------------------------------------------------------------------------------------------------------- the program
def _drift_clip(seed=0):
    """Random 5 x 5 blocks that change from frame to frame and a brightness that drifts in time: patches resemble each other,
    and the clip itself does not loop - its last frames are brighter than its first by far more than a frame step."""
    rng = np.random.default_rng(seed)
    n, h, w = SHAPE
    base = rng.standard_normal((1, h // 5 + 1, w // 5 + 1, 3)) + 0.3 * rng.standard_normal((n, h // 5 + 1, w // 5 + 1, 3))
    big = np.kron(base, np.ones((1, 5, 5, 1)))[:, :h, :w]
    return np.clip(big * 30 + 60 + 25 * np.arange(n)[:, None, None, None], 0, 255).astype(np.uint8)


def _child(args, cwd, timeout=120):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m"] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (args[0], r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    return r


def _generate(tmp, out, extra):
    path = os.path.join(tmp, "clip.npy")
    if not os.path.exists(path):
        np.save(path, _drift_clip())
    _child(["hp_vae_gan_amd.generate_patchnn", "--video-path", path, "--out", os.path.join(tmp, out)] + extra, tmp)
    with open(os.path.join(tmp, out, "patchnn.json")) as f:
        return np.load(os.path.join(tmp, out, "samples.npy")), json.load(f)


@pytest.mark.parametrize("search", ["exact", "patchmatch"])
def test_program_makes_loops_whose_seam_is_better_than_without_the_flag(tmp_path, search, capsys):
    tmp = str(tmp_path)
    common = ["--num-samples", "2", "--iters", "3", "--noise", "3", "--search", search]
    a, info = _generate(tmp, "a", common + ["--wrap", "t"])
    b, _ = _generate(tmp, "b", common + ["--wrap", "t"])
    c, plain_info = _generate(tmp, "c", common)
    assert a.shape == (2,) + SHAPE + (3,) and a.dtype == np.uint8
    assert np.array_equal(a, b)                                     # equal bytes on every run
    assert info["wrap"] == "t" and "wrap" not in plain_info
    assert not np.array_equal(a, c)
    clip = os.path.join(tmp, "clip.npy")
    ring = evaluate.evaluate(samples=os.path.join(tmp, "a", "samples.npy"), real=clip, out=os.path.join(tmp, "ea"), wrap="t")
    flat = evaluate.evaluate(samples=os.path.join(tmp, "c", "samples.npy"), real=clip, out=os.path.join(tmp, "ec"), wrap="t")
    assert ring["wrap"] == "t" and ring["seam_seconds"] > 0
    real = _drift_clip()
    for smp, got in zip(a, ring["per_sample"]):
        assert (got["seam_patches"], got["seam_coherence"]) == seam_ref(smp, real, (3, 7, 7), (1, 0, 0))
        assert got["seam_patches"] == 2 * 34 * 50
    assert ring["seam_coherence"] == sum(p["seam_coherence"] for p in ring["per_sample"]) / 2
    with open(os.path.join(tmp, "ea", "metrics.json")) as f:
        assert json.load(f)["seam_coherence"] == ring["seam_coherence"]
    with capsys.disabled():
        print("\n[patchwrap] %s: seam_coherence with --wrap t %.6f, without %.6f; coherence %.6f / %.6f"
              % (search, ring["seam_coherence"], flat["seam_coherence"], ring["coherence"], flat["coherence"]))
    assert ring["seam_coherence"] < flat["seam_coherence"]          # two runs of the code against each other: no threshold
    # without the flag evaluate reports what it always did
    none = evaluate.evaluate(samples=os.path.join(tmp, "c", "samples.npy"), real=clip, out=os.path.join(tmp, "en"))
    assert not any(k in none for k in ("seam_coherence", "wrap", "seam_seconds")) and "seam_patches" not in none["per_sample"][0]
    assert none["coherence"] == flat["coherence"]
