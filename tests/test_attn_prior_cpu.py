"""Preconditions of tests/test_attn_prior_edges_gpu.py, held on the numpy restatement alone
(tests/attn_prior_cases.py), so that the GPU tests cannot pass vacuously: every case decisive in
its codes and in its alignment votes, the prior visible in what the GPU tests compare, and each
named edge visited by the restatement's own `att`. If a generator change breaks a condition, that
case's seed changes; the condition does not.
"""
import numpy as np
import pytest

import attn_prior_cases as ap
from parity import compare_forced
from test_decode_gpu import BF16_HIDDEN_TOL, BF16_TIE_EPS
from text_edges import FAMILY_MIN_SENSITIVITY


@pytest.fixture(scope="module")
def ma():
    import magpie_amd
    return magpie_amd


@pytest.fixture(scope="module")
def model64(small_model):
    return ap.mi.Magpie(small_model)


def _decisive(ref, steps, what):
    assert len(ref["codes"]) == steps, f"{what}: {len(ref['codes'])} frames"
    mg = float(ref["margins"].min())
    ag = float(ref["amargins"].min()) if len(ref["amargins"]) else float("inf")
    print(f"{what}: min margin {mg:.3g}, min alignment gap {ag:.3g}, att {ref['att'].tolist()}")
    assert mg >= ap.MIN_MARGIN, f"{what}: min margin {mg:.3g}: change this case's seed"
    assert ag >= ap.MIN_ALIGN_MARGIN, f"{what}: min alignment gap {ag:.3g}: change this case's seed"


def _moved(ref, plain, T, W, what):
    dc, da = int((ref["codes"] != plain["codes"]).sum()), int((ref["att"] != plain["att"]).sum())
    print(f"{what}: {dc} codes and {da} att entries differ from the prior-off run")
    if T > W + 2:
        assert dc >= 1, what
        assert da >= 1 or W == 0, what  # W = 0: the window is the position a alone, att is 0 in any run
        if W == 0:
            assert not ref["att"].any() and not plain["att"].any()


@pytest.mark.parametrize("T,W,seed", ap.EDGES)
def test_text_edges_are_decisive_and_moved_by_the_prior(ma, model64, T, W, seed):
    ref, plain = ap.reference(model64, ma, T, W, 0, 0, ap.EDGE_STEPS, seed)
    _decisive(ref, ap.EDGE_STEPS, f"T {T} W {W}")
    _moved(ref, plain, T, W, f"T {T} W {W}")


@pytest.mark.parametrize("name,T,xa,W,start,steps,seed", ap.WINDOWS, ids=[c[0] for c in ap.WINDOWS])
def test_window_edges_are_visited(ma, model64, name, T, xa, W, start, steps, seed):
    ref, plain = ap.reference(model64, ma, T, W, start, 0, steps, seed)
    _decisive(ref, steps, name)
    if start <= steps:
        _moved(ref, plain, T, W, name)
    else:  # lp all zero throughout: the plain run
        assert np.array_equal(ref["codes"], plain["codes"]) and np.array_equal(ref["att"], plain["att"])
    att, jump = ref["att"], ref["att"] - ref["base"]
    if name == "a_reaches_the_end":
        assert int((att == T - 1).sum()) >= 3  # arrives, then stays for >= 2 frames
    if name.startswith("wide_window"):
        assert jump.max() >= 64  # a winner in waves 1+
    if name == "strided_window":
        far = max(float(w[256:].max() / w.max()) for w in ref["avg"] if len(w) > 256)
        print(f"{name}: largest jump {int(jump.max())}; the best avg entry at offset >= 256 is {far:.3g} of its window's winner")
        assert W >= 256 and any(len(w) > 256 for w in ref["avg"])
        assert jump.max() >= 256 or far >= 0.1
        assert (jump.max() >= 256) == ap.STRIDED_WINNER_PAST_256  # what the table records
    if name == "window_wider_than_the_text":
        assert W > T and (ref["base"] >= 2).any()  # hi clipped from the start; lp non-zero once a >= 2


@pytest.mark.parametrize("T,xa,W", ap.TIED_CASES)
def test_tied_votes_are_exact_ties(ma, small_model, T, xa, W):
    """K = V = 0: every window entry of every frame is the same number, the window spans four
    waves, and the first index of the maximum is a = 0 throughout"""
    M = ap.mi.Magpie(ap.tied_model(small_model))
    r = ap.restate(M, ap.tokens(ma, T, ap.TIED_SEED), 0, ap.TIED_STEPS, ap.EPS, W, ignore_eos=True)
    assert len(r["codes"]) == ap.TIED_STEPS and not r["att"].any()
    assert all(len(w) >= 193 and np.ptp(w) == 0.0 for w in r["avg"])


def test_full_depth_fixture(ma):
    """tests/golden/attn_prior_full.npz: the four masks, their tokens the table's, decisive, moved
    by the prior. The stored results are restate()'s as it stood when the fixture was written:
    after any change to restate(), rerun tests/golden/make_attn_prior.py."""
    g = np.load(ap.GOLD_FULL)
    for i, (mask, W, seed) in enumerate(ap.FULL_CASES):
        assert int(g[f"m{i}_mask"]) == mask and int(g[f"m{i}_W"]) == W
        assert np.array_equal(g[f"m{i}_tokens"], ap.tokens(ma, ap.FULL_T, seed))
        ref = {k: g[f"m{i}_{k}"] for k in ("codes", "att", "margins", "amargins")}
        plain = {"codes": g[f"m{i}_plain_codes"], "att": g[f"m{i}_plain_att"]}
        _decisive(ref, ap.FULL_STEPS, f"12 layers, mask {mask:#x}")
        _moved(ref, plain, ap.FULL_T, W, f"12 layers, mask {mask:#x}")
        assert g[f"m{i}_hidden"].shape == (ap.FULL_STEPS, 768) and len(g[f"m{i}_tokens"]) == ap.FULL_T
    assert [bin(c[0]).count("1") for c in ap.FULL_CASES] == [12, 5, 3, 1]


@pytest.mark.parametrize("T", sorted(ap.CFG_SEEDS))
def test_guided_cases_are_decisive_and_need_the_partner(ma, model64, T):
    """scale 2.5 with the prior: no near-tie, and the partner's logits matter: with the partner's
    row replaced by the conditional one at least one code changes"""
    ref = ap.cfg_reference(model64, ma, T)
    _decisive(ref, ap.CFG_STEPS, f"guided T {T}")
    alone = ap.restate(model64, ap.tokens(ma, T, ap.CFG_SEEDS[T]), 0, ap.CFG_STEPS, ap.EPS, 5, cfg_scale=ap.CFG_SCALE,
                       ignore_eos=True, partner_is_cond=True)
    n = min(len(alone["codes"]), ap.CFG_STEPS)
    assert (alone["codes"][:n] != ref["codes"][:n]).any()
    assert np.abs(ref["hidden_uncond"] - ref["hidden"]).max() > 1e-2  # a different branch
    plain = ap.restate(model64, ap.tokens(ma, T, ap.CFG_SEEDS[T]), 0, ap.CFG_STEPS, None, 5, cfg_scale=ap.CFG_SCALE,
                       ignore_eos=True)
    _moved(ref, plain, T, 5, f"guided T {T}")  # a device that ignored the prior under guidance would miss


# ---------------------------------------------------------------- bf16
@pytest.mark.parametrize("T,xa,W,seed", ap.BF16_CASES)
def test_bf16_restatement_agrees_with_the_oracle(ma, oracle, small_model, model64, T, xa, W, seed):
    """prior off, teacher forced along the oracle mode 1's own codes: hidden states within
    BF16_RESTATE_SPREAD, a fifth of BF16_HIDDEN_TOL = 3e-2 (measured 7.0e-5 at T = 70 and 4.6e-3 at
    T = 200: the oracle keeps f32 intermediates, so an activation's bf16 rounding can fall the
    other way), and every differing decision is one of the oracle's near-ties"""
    tok = ap.tokens(ma, T, seed)
    om = oracle.Model(small_model)
    try:
        om.set_weight_mode(1)
        o = om.synthesize(tok, speaker=0, max_steps=ap.BF16_STEPS, ignore_eos=True, trace=True)
    finally:
        om.close()
    r = ap.restate(model64, tok, 0, ap.BF16_STEPS, None, W, forced=(o["codes"], None), bf16=True, ignore_eos=True)
    d = float(np.abs(r["hidden"] - o["hidden"][:ap.BF16_STEPS]).max())
    print(f"bf16 T {T}: restatement vs oracle mode 1: hidden {d:.3g}")
    assert d <= ap.BF16_RESTATE_SPREAD and 5 * ap.BF16_RESTATE_SPREAD <= BF16_HIDDEN_TOL
    compare_forced(r["codes"], {"codes": o["codes"], "margins": o["margins"][:ap.BF16_STEPS]}, tie_eps=BF16_TIE_EPS,
                   max_ties=ap.BF16_MAX_TIES)


def test_bf16_cases_can_fail_and_votes_are_clear(ma, model64):
    """The prior moves a compared hidden state by >= 3 x BF16_HIDDEN_TOL (text_edges.py's
    FAMILY_MIN_SENSITIVITY rule); ALIGN_TIE_BF16 is twice the largest shift of any window avg
    entry between the bf16 restatement accumulating in f32 and in f64 over the bf16 cases
    (ALIGN_SHIFT_BF16, measured here); at most 1 vote in 12 is nearer than that."""
    shift = 0.0
    for T, xa, W, seed in ap.BF16_CASES:
        tok = ap.tokens(ma, T, seed)
        r = ap.restate(model64, tok, 0, ap.BF16_STEPS, ap.EPS, W, bf16=True, ignore_eos=True)
        assert len(r["codes"]) == ap.BF16_STEPS
        forced = (r["codes"], r["att"])
        off = ap.restate(model64, tok, 0, ap.BF16_STEPS, None, W, forced=forced, bf16=True, ignore_eos=True)
        moved = float(np.abs(off["hidden"] - r["hidden"]).max())
        r32 = ap.restate(model64, tok, 0, ap.BF16_STEPS, ap.EPS, W, forced=forced, bf16=True, ignore_eos=True, acc32=True)
        s = max(float(np.abs(a - b).max()) for a, b in zip(r["avg"], r32["avg"]))
        shift = max(shift, s)
        near = int((r["amargins"] < ap.ALIGN_TIE_BF16).sum())
        print(f"bf16 T {T}: the prior moves the hidden state by {moved:.3g}; avg shift f32 vs f64 accumulation {s:.3g}; "
              f"{near} of {len(r['amargins'])} votes under ALIGN_TIE_BF16; smallest gap {r['amargins'].min():.3g}")
        assert moved >= FAMILY_MIN_SENSITIVITY * BF16_HIDDEN_TOL
        assert near <= 1
    print(f"largest avg shift {shift:.3g} (recorded ALIGN_SHIFT_BF16 {ap.ALIGN_SHIFT_BF16:g})")
    assert shift <= ap.ALIGN_SHIFT_BF16 and ap.ALIGN_TIE_BF16 == 2 * ap.ALIGN_SHIFT_BF16
