"""`generate_patchnn --search patchmatch` on the GPU: one and two patchnn_refine steps against the numpy composition (reference
PatchMatch searches, patchnn_weights, the vote reference), and the program itself, each run a fresh child process under its own
timeout (a failed child ends the test): the files it writes, equal bytes on a second run, seeds, retargeting, and
`--search exact` against no flag at all."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from hp_vae_gan_amd import generate_patchnn  # noqa: E402
from patchmatch_ref import patch_match_ref  # noqa: E402
from test_patchgen import vote_ref  # noqa: E402
from test_patchnn import _rand  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
SHAPE = (5, 40, 56)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------------------- one refine step
def _step_ref(query, keys, values, patch, alpha_abs, iters, seed, fwd, rev):
    """(result, fwd field, rev field, seed after) of one PatchMatch step, in numpy."""
    if np.isinf(alpha_abs):
        nn = patch_match_ref(query, keys, patch, iters, seed, None, fwd)[1]
        return vote_ref(values, nn, patch, query)[0], nn, None, seed + 1
    m, rnn, _ = patch_match_ref(keys, query, patch, iters, seed, None, rev)
    w = np.float32(1.0) / (m.astype(np.float32) + np.float32(alpha_abs))
    assert w.dtype == np.float32
    nn = patch_match_ref(query, keys, patch, iters, seed + 1, w.reshape(-1), fwd)[1]
    return vote_ref(values, nn, patch, query)[0], nn, rnn, seed + 2


@pytest.mark.parametrize("alpha", [0.005, float("inf")])
def test_refine_steps_equal_the_numpy_composition(alpha):
    """The first step starts both searches from the hash (a fresh state: seeds 0 and 1); the second starts from the first step's
    fields, under the next seeds of the state."""
    query, keys, values, patch = _rand((5, 20, 28), 1), _rand((4, 19, 31), 2), _rand((4, 19, 31), 3), (3, 7, 7)
    alpha_abs = alpha * 441 * 255 * 255
    want1, fwd, rev, seed = _step_ref(query, keys, values, patch, alpha_abs, 2, 0, None, None)
    got1 = generate_patchnn.patchnn_refine(_dev(query), _dev(keys), _dev(values), patch, alpha_abs, search="patchmatch", pm_iters=2)
    assert got1.dtype == torch.uint8 and np.array_equal(got1.cpu().numpy(), want1)
    assert (want1 != query).any()
    # with a state: the same first step, then a second one on its result
    state = generate_patchnn.patchnn_search_state(seed=0, index=0)
    a = generate_patchnn.patchnn_refine(_dev(query), _dev(keys), _dev(values), patch, alpha_abs, search="patchmatch", pm_iters=2,
                                        state=state)
    assert torch.equal(a, got1)
    assert np.array_equal(state["fwd"].cpu().numpy(), fwd) and state["count"] == seed
    assert (state["rev"] is None) == np.isinf(alpha) and (rev is None or np.array_equal(state["rev"].cpu().numpy(), rev))
    want2 = _step_ref(want1, keys, values, patch, alpha_abs, 2, seed, fwd, rev)[0]
    b, score = generate_patchnn.patchnn_refine(a, _dev(keys), _dev(values), patch, alpha_abs, return_score=True, search="patchmatch",
                                               pm_iters=2, state=state)
    assert np.array_equal(b.cpu().numpy(), want2) and np.isfinite(score) and score >= 0
    # below pm_from_level the step is the exact one, and it leaves its fields in the state
    exact = generate_patchnn.patchnn_refine(_dev(query), _dev(keys), _dev(values), patch, alpha_abs)
    st = generate_patchnn.patchnn_search_state()
    low = generate_patchnn.patchnn_refine(_dev(query), _dev(keys), _dev(values), patch, alpha_abs, search="patchmatch", pm_iters=2,
                                          pm_from_level=2, level=1, state=st)
    assert torch.equal(low, exact) and st["count"] == 0 and st["fwd"].numel() == 3 * 14 * 22
    assert not torch.equal(exact, got1)


def test_sample_seed_rule():
    s = generate_patchnn.patchnn_search_state(seed=3, index=2)
    assert (s["base"], s["count"], s["fwd"], s["rev"]) == (5 * 1000003, 0, None, None)


# ----------------------------------------------------------------------------------------------------------- the program
def _blocks(seed=0):
    """Random 5 x 5 blocks, so patches resemble each other (test_patchgen_program_gpu.py's clip at this size)."""
    rng = np.random.default_rng(seed)
    n, h, w = SHAPE
    base = rng.standard_normal((n, h // 5 + 1, w // 5 + 1, 3))
    big = np.kron(base, np.ones((1, 5, 5, 1)))[:, :h, :w]
    return np.clip(big * 50 + 128, 0, 255).astype(np.uint8)


def _child(args, cwd, timeout=120):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m"] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (args[0], r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    return r


def _generate(tmp, out, extra):
    path = os.path.join(tmp, "clip.npy")
    if not os.path.exists(path):
        np.save(path, _blocks())
    _child(["hp_vae_gan_amd.generate_patchnn", "--video-path", path, "--out", os.path.join(tmp, out)] + extra, tmp)
    with open(os.path.join(tmp, out, "patchnn.json")) as f:
        return np.load(os.path.join(tmp, out, "samples.npy")), json.load(f)


# at the default noise a clip this small can come back as itself whatever the seed (see test_patchgen_program_gpu.py)
PM = ["--search", "patchmatch", "--num-samples", "2", "--iters", "3", "--pm-iters", "2", "--noise", "3"]


def test_program_writes_repeats_and_follows_the_seed(tmp_path):
    tmp = str(tmp_path)
    a, info = _generate(tmp, "a", PM + ["--seed", "3"])
    b, _ = _generate(tmp, "b", PM + ["--seed", "3"])
    assert a.shape == (2,) + SHAPE + (3,) and a.dtype == np.uint8
    assert np.array_equal(a, b)                                       # a seed gives the same bytes on every run
    assert not np.array_equal(a[0], a[1])                             # sample i runs under seed + i
    real = _blocks()
    assert a.min() >= real.min() and a.max() <= real.max()
    assert (info["search"], info["pm_iters"], info["pm_from_level"]) == ("patchmatch", 2, 1)
    assert info["level_sizes"] == [[5, 17, 24], [5, 23, 32], [5, 30, 42], [5, 40, 56]] and info["iters"] == 3
    assert len(info["final_score_per_sample"]) == 2 and all(np.isfinite(v) and v >= 0 for v in info["final_score_per_sample"])
    assert sorted(n for n in os.listdir(os.path.join(tmp, "a")) if n.startswith("sample_")) == ["sample_0000.gif", "sample_0001.gif"]


def test_program_retargets_and_takes_its_defaults(tmp_path):
    """--size with another width: the guess's and the keys' grids differ at every level, and the fields are carried between
    them.  No --pm-* flag: 4 iterations from level 1."""
    s, info = _generate(str(tmp_path), "r", ["--search", "patchmatch", "--num-samples", "1", "--iters", "2", "--size", "5", "40", "72"])
    assert s.shape == (1, 5, 40, 72, 3) and s.dtype == np.uint8
    assert info["size"] == [5, 40, 72] and (info["search"], info["pm_iters"], info["pm_from_level"]) == ("patchmatch", 4, 1)


def test_search_exact_is_the_program_without_the_flag(tmp_path):
    tmp = str(tmp_path)
    common = ["--num-samples", "1", "--iters", "2", "--min-size", "30", "--seed", "4"]
    a, ia = _generate(tmp, "a", common)
    b, ib = _generate(tmp, "b", common + ["--search", "exact"])
    assert np.array_equal(a, b)
    for info in (ia, ib):
        info.pop("seconds_per_sample")
        assert not any(k in info for k in ("search", "pm_iters", "pm_from_level"))
    assert ia == ib and ia["iters"] == 2 and ia["seed"] == 4
