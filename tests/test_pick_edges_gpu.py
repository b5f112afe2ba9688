"""The code pick at every edge, on the device (tests/pick_cases.py: the crafted-logit models,
the case table, the margin rule; tests/test_pick_edges_cpu.py holds the table's preconditions).

Every logit row of a crafted file is known exactly, so every decision of every run has one expected
code, whatever came before it: all decisions of a run are compared, none is skipped after a
first difference. A decision may differ only where its row is not flat and the oracle's draw
margin is under the project's bar of 1e-5; the argmax never.

  lt_sample       mp_hip_lt_sample over the whole table, forbid_eos both ways (f32; Q8 on the k edges)
  pick sites      decode runs of every mode and batch size that picks somewhere else
  first-max       greedy runs on duplicated maxima, the stop rule at EOS
  EOS sampled     the run ends on a sampled EOS that is not the argmax
  moved ids       the general per-row mask
  guidance        cfg_mix under ties
  limits          top_k 0 and 2025 refused when sampling, accepted when greedy
"""
import numpy as np
import pytest

import pick_cases as pc

pytestmark = pytest.mark.gpu

SOURCE_OF = {"f32": "small", "bf16": "small", "f16": "f16", "q8": "q8", "q4": "q4"}
SITES = [("f32", 1), ("f32", 3), ("f32", 8), ("bf16", 1), ("bf16", 2), ("bf16", 5), ("bf16", 16), ("bf16", 32), ("f16", 1),
         ("f16", 16), ("q8", 1), ("q8", 16), ("q4", 1)]
FULL = {("f32", 1), ("f32", 3), ("bf16", 16)}  # the modes that take the whole k list


@pytest.fixture(scope="module")
def ma():
    import magpie_amd
    if magpie_amd.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    return magpie_amd


@pytest.fixture(scope="module")
def sources(ma, small_model, q8_model, q4_model, f16_model):
    return {"small": small_model, "q8": q8_model, "q4": q4_model, "f16": f16_model, "moved": pc.moved_source(ma)}


@pytest.fixture(scope="module")
def devices(ma, sources):
    """device(source, file, weights): one Device per crafted file and weight mode, kept for the
    module; it counts its mp_hip_lt_sample calls (the draw's step index is 4 + that count)"""
    held = {}

    def device(source, name, weights="f32"):
        key = (source, name, weights)
        if key not in held:
            held[key] = ma.Device(pc.crafted(sources[source], name), weights=weights)
            held[key].lt_calls = 0
        return held[key]

    yield device
    for d in held.values():
        d.close()


@pytest.fixture(scope="module")
def oracle_runs(oracle, ma, sources):
    """run(source, case, stream): oracle.Model(crafted file).synthesize of a case, computed once
    and held equal to the rows' own simulation (pick_cases.expected_run)"""
    models, runs = {}, {}

    def run(source, case, stream):
        key = (source, case["id"], stream)
        if key not in runs:
            if (source, case["file"]) not in models:
                models[(source, case["file"])] = oracle.Model(pc.crafted(sources[source], case["file"]))
            o = models[(source, case["file"])].synthesize(_tokens(ma, stream), max_steps=case["frames"], ignore_eos=case["ignore_eos"],
                                                          trace=False, temperature=case["T"], top_k=case["k"], seed=case["seed"],
                                                          stream=stream)
            sim = _sim(oracle, case, stream)
            assert o["n_frames"] == sim["n_frames"] and np.array_equal(o["codes"], sim["codes"]), key
            runs[key] = o
        return runs[key]

    yield run
    for m in models.values():
        m.close()


def _tokens(ma, b):
    return ma.synthetic_tokens(6 + b % 5, seed=900 + b)


def _sim(oracle, case, stream, scale=None):
    return pc.expected_run(oracle, case["file"], case["T"], case["k"], case["ignore_eos"], case["seed"], stream, case["frames"], scale)


def _hold(codes, want, margins, pats, what):
    """every decision of codes [n][8] against `want` under the margin rule: (decisions, excused)"""
    codes, want = np.asarray(codes).reshape(-1, 8), np.asarray(want).reshape(-1, 8)
    assert codes.shape == want.shape, f"{what}: {codes.shape} against {want.shape}"
    excused = 0
    for f, cb in np.argwhere(codes != want):
        mg = float(np.asarray(margins).reshape(-1, 8)[f, cb])
        assert pats[cb] != "flat" and mg < pc.BAR, (f"{what}: frame {f} cb {cb} ({pats[cb]}): device {codes[f, cb]}, "
                                                    f"expected {want[f, cb]}, draw margin {mg:.3g}")
        excused += 1
    return codes.size, excused


def _decode(ma, dev, case, B, frames=None, **kw):
    toks = [_tokens(ma, b) for b in range(B)]
    return dev.synthesize(toks, speakers=[b % 5 for b in range(B)], max_dec_steps=frames or case["frames"],
                          temperature=case["T"], top_k=case["k"], seed=case["seed"], ignore_eos=case["ignore_eos"], **kw)


def _hold_run(oracle, r, case, slots, what, scale=None):
    pats = pc.rows_of(case["file"])[1]
    n = ex = 0
    for b in slots:
        sim = _sim(oracle, case, b, scale)
        assert int(r.n_frames[b]) == sim["n_frames"], f"{what} slot {b}: {int(r.n_frames[b])} frames, {sim['n_frames']} expected"
        d, e = _hold(r.codes[b], sim["codes"], sim["margins"][:sim["n_frames"]], pats, f"{what} slot {b}")
        n, ex = n + d, ex + e
    return n, ex


def _slots(B):
    return sorted({0, B - 1} | ({15, 16} if B == 32 else set()))


# ---------------------------------------------------------------- 1. mp_hip_lt_sample
def _lt_sample_case(oracle, dev, case, calls=2):
    pats = pc.rows_of(case["file"])[1]
    bos = pc.bos_of(case["file"])
    rng = np.random.default_rng(case["seed"] + 1)
    n = ex = 0
    for forbid in (False, True):
        for _ in range(calls):
            h = rng.standard_normal(768).astype(np.float32)
            step = 4 + dev.lt_calls
            smp, amx = dev.lt_sample(h, temperature=case["T"], top_k=case["k"], forbid_eos=forbid, seed=case["seed"])
            dev.lt_calls += 1
            es, ea, mg = pc.expected(oracle, case["file"], case["T"], case["k"], forbid, case["seed"], -1, step)
            assert np.array_equal(amx, ea), (case["id"], forbid, amx, ea)
            d, e = _hold(smp, es, mg, pats, f"{case['id']} forbid_eos {forbid} step {step}")
            n, ex = n + d + 8, ex + e
            special = [(bos <= c < bos + 8) and (forbid or c != bos + 1) for c in list(smp) + list(amx)]
            assert not any(special), (case["id"], forbid, smp, amx)
    return n, ex


@pytest.mark.parametrize("cid", list(pc.CASES))
def test_lt_sample_over_the_table(ma, oracle, devices, cid):
    case = pc.CASES[cid]
    dev = devices("moved" if case["file"] == "moved" else "small", case["file"])
    n, ex = _lt_sample_case(oracle, dev, case)
    print(f"{cid}: {n} decisions, {ex} under the bar")
    assert n == 64 and ex <= 2


def test_lt_sample_q8_k_edges(ma, oracle, devices):
    dev = devices("q8", "kedge", "q8")
    n = ex = 0
    for cid in pc.K_SWEEP:
        d, e = _lt_sample_case(oracle, dev, pc.CASES[cid], calls=1)
        n, ex = n + d, ex + e
    print(f"Q8 k edges: {n} decisions, {ex} under the bar")
    assert n == 32 * len(pc.KS) and ex <= 4


# ---------------------------------------------------------------- 2. every pick site
def _site_cases(ma, oracle, devices, oracle_runs, weights, B, cids, last_too):
    source = SOURCE_OF[weights]
    n = ex = 0
    for cid in cids:
        case = pc.CASES[cid]
        r = _decode(ma, devices(source, case["file"], weights), case, B)
        d, e = _hold_run(oracle, r, case, _slots(B), f"{weights} B {B} {cid}")
        n, ex = n + d, ex + e
        # the oracle's own run of this file
        for b in {0, B - 1} if last_too else {0}:
            o = oracle_runs(source, case, b)
            d2, _ = _hold(r.codes[b], o["codes"], _sim(oracle, case, b)["margins"], pc.rows_of(case["file"])[1], f"{cid} slot {b}")
            assert d2 == 8 * case["frames"]
    print(f"{weights} B {B}: {len(cids)} cases, {n} decisions, {ex} under the bar")
    assert n == len(cids) * len(_slots(B)) * 16 * 8
    return n, ex


@pytest.mark.parametrize("weights,B", SITES, ids=[f"{w}-B{b}" for w, b in SITES])
def test_every_pick_site(ma, oracle, devices, oracle_runs, weights, B):
    """flat k = 80, gauss, straddle k = 64 and 80, two-level m = 70 k = 80, gauss k = 65 and the
    greedy first-max rows, slot 0 and the last slot against the oracle's run of the same file"""
    n, ex = _site_cases(ma, oracle, devices, oracle_runs, weights, B, pc.EVERYWHERE, True)
    assert ex <= 2


K_LIST = [c for c in pc.CASES if c.startswith("k") and c not in pc.EVERYWHERE]
K_CHUNKS = [K_LIST[i:i + 5] for i in range(0, len(K_LIST), 5)]


@pytest.mark.parametrize("chunk", range(len(K_CHUNKS)))
@pytest.mark.parametrize("weights,B", sorted(FULL), ids=[f"{w}-B{b}" for w, b in sorted(FULL)])
def test_full_k_list(ma, oracle, devices, oracle_runs, weights, B, chunk):
    """every k of the table (T = 0.7, and T = 100 at the row and mask boundaries), slot 0 against
    the oracle's run; the dense decisions' expected share under the bar is 4 %"""
    n, ex = _site_cases(ma, oracle, devices, oracle_runs, weights, B, K_CHUNKS[chunk], False)
    assert ex <= max(2, n // 100)


# ---------------------------------------------------------------- 3. greedy first-max
@pytest.mark.parametrize("weights,B", [("f32", 1), ("f32", 3), ("bf16", 1), ("bf16", 2), ("q8", 1)])
def test_greedy_first_max(ma, oracle, devices, oracle_runs, weights, B):
    source = SOURCE_OF[weights]
    n = 0
    for f in ("firstmax_a", "firstmax_b"):
        for cid in (f"{f}_greedy", f"{f}_greedy_eos_live"):
            case = pc.CASES[cid]
            r = _decode(ma, devices(source, f, weights), case, B)
            rows = pc.rows_of(f)[0]
            for b in range(B):
                assert int(r.n_frames[b]) == case["frames"], f"{cid}: (2015, EOS) tied: the first is 2015, the run goes on"
                for cb in range(8):
                    m = pc.masked(rows[cb], pc.BOS, case["ignore_eos"])
                    first = int(np.nonzero(m == m.max())[0][0])
                    assert (r.codes[b][:, cb] == first).all(), (cid, b, cb, first, r.codes[b][:, cb])
                    n += case["frames"]
            assert np.array_equal(r.codes[0], oracle_runs(source, case, 0)["codes"])
    case = pc.CASES["firstmax_eos_stops"]
    r = _decode(ma, devices(source, "firstmax_eos", weights), case, B)
    o = oracle_runs(source, case, 0)
    assert o["n_frames"] == 4
    for b in range(B):
        assert int(r.n_frames[b]) == 4
        d, _ = _hold(r.codes[b], o["codes"], o["margins"][:4], ["first_max"] * 8, f"EOS the maximum, slot {b}")
        n += d
    assert n == B * (4 * 8 * 16 + 32)


# ---------------------------------------------------------------- 4. EOS sampled, not the argmax
def test_eos_sampled_not_argmax(ma, oracle, devices, oracle_runs):
    case = pc.CASES["eos_sampled"]
    want = [oracle_runs("small", case, s) for s in pc.EOS_SAMPLED_STREAMS]
    assert len({o["n_frames"] for o in want}) == 2 and all(4 <= o["n_frames"] < case["frames"] for o in want)
    pats = pc.rows_of("eos3")[1]
    n = 0
    r = _decode(ma, devices("small", "eos3"), case, 1)
    assert int(r.n_frames[0]) == want[0]["n_frames"]
    n += _hold(r.codes[0], want[0]["codes"], want[0]["margins"], pats, "f32 B 1")[0]
    r = _decode(ma, devices("small", "eos3", "bf16"), case, 2)
    for b in (0, 1):
        assert int(r.n_frames[b]) == want[b]["n_frames"], b
        n += _hold(r.codes[b], want[b]["codes"], want[b]["margins"], pats, f"bf16 B 2 slot {b}")[0]
    assert n == 8 * (2 * want[0]["n_frames"] + want[1]["n_frames"])


# ---------------------------------------------------------------- 5. moved ids
@pytest.mark.parametrize("weights,B", [("f32", 1), ("f32", 3), ("bf16", 2)])
def test_moved_ids(ma, oracle, devices, oracle_runs, weights, B):
    n = ex = 0
    for cid in ("moved_greedy", "moved_k80", "moved_k2016"):
        case = pc.CASES[cid]
        r = _decode(ma, devices("moved", "moved", weights), case, B)
        d, e = _hold_run(oracle, r, case, range(B), f"{weights} B {B} {cid}")
        n, ex = n + d, ex + e
        assert np.array_equal(r.codes[0], oracle_runs("moved", case, 0)["codes"]) or e
        for b in range(B):
            c = r.codes[b]
            assert not ((c >= pc.MOVED_BOS) & (c < pc.MOVED_BOS + 8)).any(), (cid, b)
    # EOS live: (1001, 1008) tied in codebook 3, EOS the first from frame 4 on
    case = dict(pc.CASES["moved_greedy"], ignore_eos=False)
    r = _decode(ma, devices("moved", "moved", weights), case, B)
    assert [int(v) for v in r.n_frames] == [4] * B and _sim(oracle, case, 0)["n_frames"] == 4
    assert n == 3 * B * 16 * 8 and ex <= 2


# ---------------------------------------------------------------- 6. guidance
@pytest.mark.parametrize("weights,B", [("f32", 2), ("bf16", 9)])
def test_guided_pick_under_ties(ma, oracle, devices, weights, B):
    n = ex = 0
    for cid in pc.GUIDED:
        case = pc.CASES[cid]
        dev = devices("small", case["file"], weights)
        try:
            plain = _decode(ma, dev, case, B)
            for scale in pc.GUIDED_SCALES:
                dev.set_cfg(scale)
                r = _decode(ma, dev, case, B)
                d, e = _hold_run(oracle, r, case, sorted({0, B - 1, min(B - 1, 7)}), f"{weights} B {B} {cid} scale {scale}", scale)
                n, ex = n + d, ex + e
            dev.set_cfg(1.0)
            one = _decode(ma, dev, case, B)
            for b in range(B):
                assert np.array_equal(one.codes[b], plain.codes[b]), (cid, b)
        finally:
            dev.set_cfg(0.0)
    assert n == len(pc.GUIDED) * 2 * len({0, B - 1, min(B - 1, 7)}) * 16 * 8 and ex <= 2


# ---------------------------------------------------------------- 7. limits stay limits
def test_top_k_limits(ma, oracle, devices):
    dev = devices("small", "kedge")
    case = pc.CASES["T0.7_gauss"]
    h = np.zeros(768, np.float32)
    n = 0
    for k in (0, 2025):
        for T in (0.01, 0.7):
            with pytest.raises(ma.MagpieError, match="MP_ERR_ARG"):
                dev.synthesize([_tokens(ma, 0)], max_dec_steps=8, temperature=T, top_k=k, ignore_eos=True)
            with pytest.raises(ma.MagpieError, match="MP_ERR_ARG"):
                dev.lt_sample(h, temperature=T, top_k=k)  # refused before the call counter moves
        # greedy: any top_k is accepted
        g = dev.synthesize([_tokens(ma, 0)], max_dec_steps=8, temperature=0.0099, top_k=k, ignore_eos=True)
        want = _sim(oracle, dict(case, T=0.0, frames=8), 0)
        assert np.array_equal(g.codes[0], want["codes"])
        n += g.codes[0].size
        # and the device is still usable
        d, _ = _lt_sample_case(oracle, dev, case, calls=1)
        n += d
    assert n == 2 * (64 + 32)
