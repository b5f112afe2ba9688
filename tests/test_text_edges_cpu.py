"""Preconditions of tests/test_text_edges_gpu.py, held on the CPU oracle alone, so that the
GPU tests cannot pass vacuously: every case decisive (no near-tie exit), the last text token
visible in what the GPU tests compare, and the bars resting on the oracle's own f32-vs-f64
spread. If a generator change breaks a condition for some T, that case's seed changes; the
condition does not.
"""
import os

import numpy as np
import pytest

import text_edges as te


@pytest.fixture(scope="module")
def ma():
    import magpie_amd
    return magpie_amd


@pytest.fixture(scope="module")
def runs(ma, oracle, small_model):
    r = te.OracleRuns(ma, oracle, small_model)
    yield r
    r.close()


@pytest.fixture(scope="module")
def group_runs(ma, oracle):
    r = te.OracleRuns(ma, oracle, te.group_model(ma))
    yield r
    r.close()


def _min_margin(o):
    return float(o["margins"][:te.STEPS].min())


@pytest.mark.parametrize("T", te.EDGES)
def test_every_edge_is_decisive(runs, T):
    """All 8 frames, finite hidden states, and the smallest top-1/top-2 margin of the 64
    decisions >= 2 x TIE_EPS: the GPU must reproduce every code."""
    o = runs.run(T)
    mg = _min_margin(o)
    print(f"T = {T}: min margin {mg:.3g} over {o['n_frames']} frames")
    assert mg >= te.MIN_MARGIN, f"T = {T}: min margin {mg:.3g} < {te.MIN_MARGIN:g}: change this case's seed"


@pytest.mark.parametrize("T", te.GROUP_T + te.GROUP_BATCH[1:])
def test_layer_group_cases_are_decisive(group_runs, T):
    """The same on the 5-layer model of the ragged XA K/V layer group."""
    mg = _min_margin(group_runs.run(T))
    print(f"5-layer model, T = {T}: min margin {mg:.3g}")
    assert mg >= te.MIN_MARGIN, f"T = {T}: min margin {mg:.3g} < {te.MIN_MARGIN:g}: change this case's seed"


@pytest.mark.parametrize("T", te.SENSITIVE_T)
def test_last_token_moves_the_hidden_state(ma, runs, T):
    """Replacing the last token moves the hidden state after the BOS step by >= 50 x HIDDEN_TOL
    (measured 0.99, 0.11, 3.1e-2, 1.2e-2, 6.8e-3, 3.6e-3, 1.29e-3 at T = 2 ... 1024): a kernel that
    drops or clamps away the last key misses the f32 hidden bar."""
    tok = te.tokens(ma, T)
    d = float(np.abs(runs.bos_hidden(te.last_token_replaced(tok), te.speaker(T)) - runs.run(T)["hidden"][0]).max())
    print(f"T = {T}: last token replaced moves the BOS-step hidden state by {d:.3g} "
          f"({d / te.HIDDEN_TOL:.0f} x HIDDEN_TOL)")
    assert d >= te.MIN_SENSITIVITY, d


@pytest.mark.parametrize("T", te.SPREAD_T)
def test_oracle_f32_accumulation_spread(ma, oracle, runs, small_model, T):
    """The oracle accumulating in f32 against itself in f64: identical codes, hidden states and
    encoder output within 1e-5 (measured at most 3.4e-6 and 7.7e-6). The 2e-5 bars of the GPU
    tests are 2 x that assertion."""
    ref, enc = runs.run(T), runs.encode(T)
    threads = min(16, os.cpu_count() or 1)
    oracle.set_mode(acc64=False, gelu_f16=False, threads=threads)
    try:
        m32 = oracle.Model(small_model)
        try:
            o = m32.synthesize(te.tokens(ma, T), speaker=te.speaker(T), max_steps=te.STEPS, ignore_eos=True, trace=True)
            e = m32.encode(te.tokens(ma, T))
        finally:
            m32.close()
    finally:
        oracle.set_mode(acc64=True, gelu_f16=False, threads=threads)  # the session's oracle fixture
    dh = float(np.abs(o["hidden"][:te.STEPS + 1] - ref["hidden"][:te.STEPS + 1]).max())
    de = float(np.abs(e - enc).max())
    print(f"T = {T}: oracle f32 vs f64 accumulation: hidden {dh:.3g}, encoder {de:.3g}")
    assert np.array_equal(o["codes"], ref["codes"])
    assert dh < te.MAX_SPREAD and de < te.MAX_SPREAD, (dh, de)


@pytest.mark.parametrize("weights,fixture,mode,T,bar", te.FAMILY_CASES,
                         ids=[f"{c[0]}-{c[3]}" for c in te.FAMILY_CASES])
def test_family_cases_can_fail(ma, oracle, request, weights, fixture, mode, T, bar):
    """A teacher-forced case of another weight family is kept only where the last token moves
    the BOS-step hidden state of the matching oracle mode by >= 3 x that family's hidden bar."""
    r = te.OracleRuns(ma, oracle, request.getfixturevalue(fixture), weight_mode=mode)
    try:
        tok = te.tokens(ma, T)
        d = float(np.abs(r.bos_hidden(te.last_token_replaced(tok), te.speaker(T)) - r.bos_hidden(tok, te.speaker(T))).max())
    finally:
        r.close()
    print(f"{weights}, T = {T}: last token replaced moves the BOS-step hidden state by {d:.3g} "
          f"({d / bar:.1f} x the {bar:g} bar)")
    assert d >= te.FAMILY_MIN_SENSITIVITY * bar, d
