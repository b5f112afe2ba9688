"""Preconditions of tests/test_pick_edges_gpu.py, held on the oracle alone (tests/pick_cases.py),
so that the GPU tests cannot pass vacuously: the crafted files' logits are the chosen rows for any
hidden state, every tie case tells the contract's tie rule from its reverse, every case's draws
visit what it is named for, and the seeds keep the margins the GPU tests' equality rests on. If a
generator change breaks a condition, that case's seed changes; the condition does not.
"""
import numpy as np
import pytest

import pick_cases as pc


@pytest.fixture(scope="module")
def ma():
    import magpie_amd
    return magpie_amd


@pytest.fixture(scope="module")
def sources(ma, small_model, q8_model, q4_model, f16_model):
    return {"small": small_model, "q8": q8_model, "q4": q4_model, "f16": f16_model, "moved": pc.moved_source(ma)}


@pytest.mark.parametrize("source,name", [(s, n) for s in pc.SOURCES for n in pc.FILES_OF[s]])
def test_crafted_logits_are_the_rows(oracle, sources, source, name):
    """lt_sample on three random hidden states equals sample_top_k on the bias rows"""
    om = oracle.Model(pc.crafted(sources[source], name))
    rng = np.random.default_rng(7)
    n = 0
    try:
        for i, (T, k, forbid) in enumerate([(0.7, 80, False), (0.7, 2024, True), (0.0, 80, False)]):
            h = rng.standard_normal(768).astype(np.float32) * (1.0 + 3.0 * i)
            smp, amx, _ = om.lt_sample(h, temperature=T, top_k=k, forbid_eos=forbid, seed=3 + i, stream=2, step=9)
            es, ea, _ = pc.expected(oracle, name, T, k, forbid, 3 + i, 2, 9)
            assert np.array_equal(smp, es) and np.array_equal(amx, ea), (source, name, T, k)
            n += 16
    finally:
        om.close()
    assert n == 48


def _decisions(oracle, case, reverse):
    """the case's picks (stream 0) under the contract (reverse False) or with the tie-break
    reversed at the k-th place and in the rank order, and `>=` in the first-max scan"""
    rows, _ = pc.rows_of(case["file"])
    out = []
    for f in range(case["frames"]):
        forbid = case["ignore_eos"] or f < 4
        for cb in pc.about_cbs(case):
            m = pc.masked(rows[cb], pc.bos_of(case["file"]), forbid)
            if np.float32(case["T"]) < np.float32(0.01):
                hit = np.nonzero(m == m.max())[0]
                out.append(int(hit[-1] if reverse else hit[0]))
            else:
                out.append(pc.np_sample(m, case["T"], case["k"], oracle.draw_u(case["seed"], 0, f, cb), reverse)[0])
    return np.array(out)


@pytest.mark.parametrize("cid", pc.TIE_CASES)
def test_tie_cases_tell_the_rules_apart(oracle, cid):
    case = pc.CASES[cid]
    fwd, rev = _decisions(oracle, case, False), _decisions(oracle, case, True)
    run = pc.expected_run(oracle, case["file"], case["T"], case["k"], case["ignore_eos"], case["seed"], 0, case["frames"])
    cbs = pc.about_cbs(case)
    n = run["n_frames"]
    assert n == case["frames"]
    assert np.array_equal(fwd.reshape(-1, len(cbs)), run["codes"][:, cbs]), "the numpy restatement is the oracle's"
    changed = int((fwd != rev).sum())
    print(f"{cid}: {changed} of {len(fwd)} decisions change under the reversed rules")
    assert changed >= case["decisive"]


@pytest.mark.parametrize("cid", list(pc.CASES))
def test_cases_visit_their_edges_and_keep_their_margins(oracle, cid):
    case = pc.CASES[cid]
    sv = pc.survey(oracle, case)
    share = sv["dense_under"] / sv["dense"] if sv["dense"] else 0.0
    print(f"{cid}: file {case['file']} T {case['T']} k {case['k']} seed {case['seed']}: {sv['decisions']} decisions, "
          f"visited {sorted(sv['visited'])}, min margin of the clear decisions {sv['min_clear']:.3g}, "
          f"{sv['dense']} dense decisions, share under {pc.BAR:g}: {share:.3f}")
    assert sv["decisions"] >= 8
    assert set(case["visits"]) <= sv["visited"], f"{cid}: visits {sorted(sv['visited'])}: change this case's seed"
    assert sv["min_clear"] >= pc.CLEAR, f"{cid}: a clear decision at margin {sv['min_clear']:.3g}: change this case's seed"
    assert share <= 0.10


def test_the_table_is_the_issue_s():
    ks = {c["k"] for c in pc.CASES.values() if c["file"] == "kedge" and c["T"] == 0.7}
    assert set(pc.KS) <= ks
    for T in pc.TS:
        assert f"T{T}_gauss" in pc.CASES and f"T{T}_peaked" in pc.CASES
    rows, pats = pc.rows_of("kedge")
    m = pc.masked(rows[pats.index("gauss_neg")], pc.BOS, True)
    top = np.sort(m)[::-1]
    assert top[39] > 0 > top[40], "40 positives: at k = 63 .. 129 the k-th value is negative and the set straddles 0"
    assert pc.masked(rows[pats.index("gauss_allneg")], pc.BOS, True).max() < 0
    g = np.sort(pc.masked(rows[pats.index("gauss")], pc.BOS, True))[::-1]
    assert g[79] > 0 and g[2014] < 0
    for name in pc.ALL_FILES:
        r = pc.rows_of(name)[0]
        assert np.isfinite(r).all() and not (r == 0).any()
    # the straddle rows: the two tie members a top-k takes are not the first two set bits in lane order
    for c in range(8):
        k = 64 if c < 4 else 80
        row, tie = pc.straddle(k, 20 + c)
        assert np.array_equal(row, pc.rows_of("straddle")[0][c])
        o = pc.order(pc.masked(row, pc.BOS, True), k + 3)
        assert list(o[k - 2:k + 3]) == tie and len({t // 64 for t in tie}) == 5
        by_lane = sorted(tie, key=lambda t: (t % 64, t // 64))
        assert set(by_lane[:2]) != set(tie[:2]) and tie[0] % 64 >= 48 and tie[1] % 64 <= 10
    for m_, cb in ((3, pats.index("two_level3")), (70, pats.index("two_level70"))):
        hi = np.nonzero(rows[cb] == rows[cb].max())[0]
        assert len(hi) == m_ and len({int(i) // 512 for i in hi}) == min(4, m_) and (np.diff(hi) > 1).any()


def test_eos_sampled_stops_where_the_simulation_says(oracle, ma, small_model):
    case = pc.CASES["eos_sampled"]
    om = oracle.Model(pc.crafted(small_model, "eos3"))
    stops = []
    try:
        for stream in pc.EOS_SAMPLED_STREAMS:
            sim = pc.expected_run(oracle, "eos3", case["T"], case["k"], False, case["seed"], stream, case["frames"])
            o = om.synthesize(ma.synthetic_tokens(8, seed=1), max_steps=case["frames"], trace=False, temperature=case["T"],
                              top_k=case["k"], seed=case["seed"], stream=stream)
            assert o["n_frames"] == sim["n_frames"] and np.array_equal(o["codes"], sim["codes"])
            assert 4 <= sim["n_frames"] < case["frames"]
            assert (sim["amax"][:, [2, 7]] == 5).all(), "EOS is never the argmax: the run stops on a sampled EOS"
            stops.append(sim["n_frames"])
    finally:
        om.close()
    print(f"eos_sampled: streams {pc.EOS_SAMPLED_STREAMS} stop at frames {stops}")
    assert len(set(stops)) == len(stops)
    # EOS the strict maximum: the greedy run stops at frame 4
    sim = pc.expected_run(oracle, "firstmax_eos", 0.0, 80, False, 0, 0, 16)
    assert sim["n_frames"] == 4


def test_mixed_rows_still_tie(oracle):
    """cfg_mix of a row with itself keeps equal logits equal (the same f32 operations on the
    same bits), so the guided cases test the same tie rule; at scale 1 the mix is the row"""
    for name in ("kedge", "straddle"):
        rows, pats = pc.rows_of(name)
        assert np.array_equal(pc.cfg_mix(rows, rows, 1.0), rows)
        for s in pc.GUIDED_SCALES:
            mixed = pc.cfg_mix(rows, rows, s)
            for cb in range(8):
                if pats[cb] == "flat":
                    assert len(np.unique(mixed[cb])) == 1
                if pats[cb].startswith("straddle"):
                    k = int(pats[cb][8:])
                    tie = pc.straddle(k, 20 + cb)[1]
                    assert len(np.unique(mixed[cb][tie])) == 1
                    o = pc.order(pc.masked(mixed[cb], pc.BOS, True), k + 3)
                    assert list(o[k - 2:k + 3]) == tie
