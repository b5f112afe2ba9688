"""The classifier-free guidance fixture (tests/golden/cfg_small.npz) kept honest without a
GPU: the restatement that wrote it (tests/golden/make_cfg.py) is, at scale 1, the plain
decode of the independent restatement (indep_small.npz), and no stored decision is a
near-tie."""
import os
import sys

import numpy as np
import pytest

from parity import TIE_EPS

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
sys.path.insert(0, GOLD)


@pytest.fixture(scope="module")
def cfg():
    return np.load(os.path.join(GOLD, "cfg_small.npz"))


def _cases(d):
    n = 0
    while f"g{n}_tokens" in d:
        n += 1
    return range(n)


def test_scale_one_is_the_plain_restatement(small_model):
    """mixed == cond at s = 1: the guided restatement gives indep_small.npz's plain codes and
    hidden states (its unconditional branch runs, and changes nothing)."""
    import make_cfg
    d = np.load(os.path.join(GOLD, "indep_small.npz"))
    m = make_cfg.Magpie(small_model)
    i = 0
    while f"c{i}_tokens" in d:
        spk, steps = (int(v) for v in d[f"c{i}_meta"])
        r = make_cfg.synthesize_cfg(m, d[f"c{i}_tokens"], spk, steps, 1.0)
        np.testing.assert_array_equal(r["codes"], d[f"c{i}_codes"])
        np.testing.assert_array_equal(r["hidden"], d[f"c{i}_hidden"])
        assert np.abs(r["hidden_uncond"] - r["hidden"]).max() > 1e-2  # a different branch
        i += 1
    assert i >= 2


def test_fixture_has_no_near_tie(cfg):
    import make_cfg
    assert make_cfg.MIN_MARGIN == 5 * TIE_EPS
    for i in _cases(cfg):
        mg = cfg[f"g{i}_margins"]
        assert mg.shape == cfg[f"g{i}_codes"].shape or len(mg) == len(cfg[f"g{i}_codes"]) + 1  # (+ an EOS frame's)
        print(f"case {i}: {len(cfg[f'g{i}_codes'])} frames, min margin {mg.min():.2e}")
        assert mg.min() >= 5 * TIE_EPS


def test_fixture_covers_the_required_cases(cfg):
    cases = list(_cases(cfg))
    scales = [float(cfg[f"g{i}_scale"]) for i in cases]
    sampled = [i for i in cases if cfg[f"g{i}_sampling"][0] >= 0.01]
    greedy = [i for i in cases if i not in sampled]
    assert len(greedy) >= 2 and len(sampled) >= 1
    assert 2.5 in [scales[i] for i in greedy] and any(scales[i] < 1.0 for i in greedy)
    assert len({len(cfg[f"g{i}_tokens"]) for i in greedy}) >= 2
    assert len({int(cfg[f"g{i}_meta"][0]) for i in greedy}) >= 2
    for i in sampled:
        assert tuple(cfg[f"g{i}_sampling"][:2]) == (0.7, 80.0)
    for i in cases:
        n = len(cfg[f"g{i}_codes"])
        assert cfg[f"g{i}_hidden"].shape[0] >= n and cfg[f"g{i}_hidden"].shape == cfg[f"g{i}_hidden_uncond"].shape
