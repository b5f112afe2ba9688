"""mp_hip_set_sampling's definition (include/magpie_hip.h) in numpy float64, the case table of
tests/test_nucleus_gpu.py, and its precondition: at most 10 % of a case's decisions fall out of the
margin rule. A decision is compared only if u S_n lies >= BAR S_n from its interval's ends, the
top-p sums on both sides of the cut >= BAR S1 from P S1 (P = 1 cuts nothing: n = n1 by definition)
and every weight >= BAR from min_p; flat rows (exact integer sums) compare at any margin."""
import numpy as np
import pytest

import pick_cases as pc


def nucleus_ref(m, T, k, P, mn, u, flat=False):
    """(code, compared, n) of one decision on the masked row m"""
    T, P, mn = (float(np.float32(v)) for v in (T, P, mn))
    o = pc.order(m, k)
    w = np.exp((m[o].astype(np.float64) - float(m[o[0]])) / T)
    n1 = int((w >= mn).sum())
    assert (w[:n1] >= mn).all(), "min-p keeps a prefix"
    cs = np.cumsum(w[:n1])
    ok = mn == 0 or np.abs(w - mn).min() >= pc.BAR
    n = n1
    if P < 1.0:
        hit = np.nonzero(cs >= P * cs[-1])[0]
        n = int(hit[0]) + 1 if len(hit) else n1
        ok = ok and min(abs(cs[n - 1] - P * cs[-1]), abs((cs[n - 2] if n > 1 else 0.0) - P * cs[-1])) >= pc.BAR * cs[-1]
    x = float(u) * cs[n - 1]
    hit = np.nonzero(x < cs[:n])[0]
    i = int(hit[0]) if len(hit) else n - 1
    ok = ok and min(x - (cs[i - 1] if i else 0.0), cs[i] - x) >= pc.BAR * cs[n - 1]
    return int(o[i]), bool(ok or flat), n


# straddle64's top-p: the cut takes two of the five equal logits at ranks 62 .. 66 (T = 0.7)
_w = np.exp(-0.01 * np.arange(62) / 0.7)
P_STRADDLE = float((_w.sum() + 1.5 * np.exp(-0.63 / 0.7)) / (_w.sum() + 5 * np.exp(-0.63 / 0.7)))
# (id, file, T, k, top_p, min_p): n = 1 and 2 (peaked gauss rows, two_level3), the 64-id row edges
# and the last row on flat rows, n = k at P = 1, the tie across the top-p edge, min_p alone with
# rank 0 and inside a run of equal weights (two_level70: w = exp(-0.5 / 0.7) = 0.4895: all or
# none), k = 1 and 2024, T = 0.01 and 100, the moved ids
CASES = [("p0.9", "kedge", 0.7, 2024, 0.9, 0.0), ("p0.5_k80", "kedge", 0.7, 80, 0.5, 0.0), ("p0.01", "kedge", 0.7, 2024, 0.01, 0.0),
         ("k1", "kedge", 0.7, 1, 0.9, 0.0), ("T0.01", "kedge", 0.01, 2024, 0.85, 0.0), ("T100", "kedge", 100.0, 2024, 0.9, 0.0),
         ("T100_p0.03", "kedge", 100.0, 2024, 0.03, 0.0), ("minp0.9", "kedge", 0.7, 2024, 1.0, 0.9),
         ("minp_out", "kedge", 0.7, 2024, 1.0, 0.49), ("minp_in", "kedge", 0.7, 2024, 0.95, 0.48),
         ("straddle_p", "straddle", 0.7, 2024, P_STRADDLE, 0.0), ("moved_p0.9", "moved", 0.7, 2024, 0.9, 0.0),
         ("moved_k80", "moved", 0.7, 80, 0.7, 0.05)] + [(f"k{k}", "kedge", 0.7, k, 1.0, 0.0) for k in (2, 63, 64, 65, 2015, 2016)]
SEED, FRAMES = 7, 8


def expected(orc, case, stream, steps):
    """(codes [len(steps)][8], compared mask, nucleus lengths) of a run of `case`, EOS forbidden"""
    _, name, T, k, P, mn = case
    rows, pats = pc.rows_of(name)
    out = np.array([[nucleus_ref(pc.masked(rows[cb], pc.bos_of(name), True), T, k, P, mn, orc.draw_u(SEED, stream, s, cb),
                                 pats[cb] == "flat") for cb in range(8)] for s in steps])
    return out[..., 0].astype(np.int32), out[..., 1].astype(bool), out[..., 2]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_at_most_a_tenth_of_a_case_falls_out(oracle, case):
    for stream, steps in [(s, range(FRAMES)) for s in (0, 15, 16, 31)] + [(-1, range(4, 4 + FRAMES))]:
        _, ok, _ = expected(oracle, case, stream, steps)
        assert (~ok).sum() <= 0.1 * ok.size, (case[0], stream, int((~ok).sum()))
