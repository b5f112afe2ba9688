"""The code pick (wave_pick_v, wave_pick_rows, pick_exchange, cfg_logit_rows / cfg_mix,
csrc/mp_fused.hpp) at its edges: the crafted-logit models, the row patterns, the case table and
the expectation helpers shared by test_pick_edges_cpu.py (the table's own preconditions, on the
oracle alone) and test_pick_edges_gpu.py (every pick site against it).

A crafted-logit model is a cached synthetic GGUF with every local_transformer_out_projections
weight zeroed and a chosen f32 row written into each bias: codebook c's logits are then bias[c]
exactly (the dot of zero weights is +0 and +0 + b == b), in every weight mode, for any hidden
state, frame, slot and text. The only thing that varies per decision is the draw
u(seed, stream, step, cb), so the expected pick of every decision is
oracle.sample_top_k(masked row, T, k, oracle.draw_u(...)), computed on the CPU, and no f32 against
f64 logit spread is left to excuse a difference. No row holds -0.0 or NaN.

The margin rule. A decision's margin is the distance of u to the nearest boundary of the
interval it fell in (oracle.sample_top_k's). The device's expf against libm's moves a boundary by
a few 1e-7 at the most; the project's draw bar is 1e-5 (test_q8_sampling_draws_exact).
  flat    the row is flat: p is 1 / k on both sides from the same float sequence, so equality
          at any margin
  clear   the draw fell in an interval >= DENSE (1e-3) wide: the table's seed leaves no such
          decision of the case's own run (stream 0, frames 0 ..) under CLEAR (1e-4)
  dense   the interval is under 1e-3 (near-uniform rows at k in the thousands, a gauss row's
          tail): no seed can clear 1e-4 over a run; such a decision may differ only under BAR,
          and the oracle alone shows that at most 10 % of a case's dense decisions lie there
          (about 4 % expected: 2 * 1e-5 / 5e-4)
On the other streams a run draws from (slots 1 .., mp_hip_lt_sample's -1) the same per-decision
rule holds: equality unless the row is not flat and the margin is under BAR.
"""
import hashlib
import os

import numpy as np

VCB = 2024
BOS, MOVED_BOS = 2016, 1000  # audio_bos of the reference's files and of the moved-ids model; EOS = bos + 1
KS = (1, 2, 63, 64, 65, 127, 128, 129, 2015, 2016, 2017, 2023, 2024)
TS = (0.0099, 0.01, 0.7, 100.0)  # 0.0099: greedy (below the 0.01 threshold)
BAR, CLEAR, DENSE = 1e-5, 1e-4, 1e-3
FAR = -40.0  # "far below": exp((FAR - max) / 0.7) ~ 1e-26, no part of any draw


def _usable(i):
    """an id that is special in neither layout"""
    return not (BOS <= i < BOS + 8 or MOVED_BOS <= i < MOVED_BOS + 8)


def _ids(rng, n, exclude=()):
    """n distinct usable ids in random (not ascending) order"""
    ex = set(int(e) for e in exclude)
    pool = [i for i in rng.permutation(VCB) if _usable(int(i)) and int(i) not in ex]
    return np.array(pool[:n], np.int64)


def _check(row):
    row = np.asarray(row, np.float32)
    assert row.shape == (VCB,) and np.isfinite(row).all()
    assert not (row == 0).any(), "no zeros (a -0.0 could hide among them)"
    return row


# ---------------------------------------------------------------- row patterns
def flat(value):
    """every logit equal: the candidates are ids 0 .. k - 1 minus the masked, p exactly uniform"""
    return _check(np.full(VCB, value, np.float32))


def two_level(m, seed, hi=1.0, near=()):
    """m ids at hi, everything else at hi - 0.5; the m ids scattered over rows and lanes, at
    least one in each 512-id wave range (m >= 4), `near`: ids that must be among them"""
    rng = np.random.default_rng(seed)
    ids = list(near)
    for w in range(min(4, m - len(ids))):  # one per wave range first, highest range first
        lo = 512 * (3 - w)
        ids.append(int(next(i for i in lo + rng.permutation(512) if i < VCB and _usable(int(i)) and i not in ids)))
    ids += [int(i) for i in _ids(rng, m - len(ids), ids)]
    row = np.full(VCB, hi - 0.5, np.float32)
    row[np.array(ids[:m])] = hi
    return _check(row), ids[:m]


def straddle(k, seed):
    """distinct, strictly descending values at ranks 0 .. k - 3, then five equal values at ranks
    k - 2 .. k + 2 in five different 64-id rows; everything else at FAR. The two that a top-k of k
    takes (lowest ids) sit in a high lane of an early row and in a low lane of a later row, the
    three it leaves in later rows at lanes 0, 1 and a middle one: a selection by lane order,
    or one that forgets the count carried across rows, takes others."""
    rng = np.random.default_rng(seed)
    rows = [int(r) for r in np.sort(rng.choice([r for r in range(1, 31) if r != MOVED_BOS // 64], 5, replace=False))]
    lanes = [int(rng.integers(48, 64)), int(rng.integers(2, 11)), 0, 1, int(rng.integers(11, 41))]
    tie = [64 * r + l for r, l in zip(rows, lanes)]
    assert all(_usable(i) for i in tie) and tie == sorted(tie)
    row = np.full(VCB, FAR, np.float32)
    top = _ids(rng, k - 2, tie)
    row[top] = (2.0 - 0.01 * np.arange(k - 2)).astype(np.float32)
    row[np.array(tie)] = np.float32(2.0 - 0.01 * (k - 2) - 0.01)
    assert len(np.unique(row[top])) == k - 2 and row[top].min() > row[tie[0]]
    return _check(row), tie


def gauss(seed, positives=None, shift=None):
    """N(0, 3^2), distinct. positives = n: shifted so that exactly n usable ids are positive
    (at k > n the k-th value is negative and the top-k set straddles 0); shift: added."""
    rng = np.random.default_rng(seed)
    row = (3.0 * rng.standard_normal(VCB)).astype(np.float32)
    if positives is not None:
        u = np.sort(row[[i for i in range(VCB) if _usable(i)]])[::-1]
        row = row - np.float32(0.5 * (float(u[positives - 1]) + float(u[positives])))
    if shift is not None:
        row = row + np.float32(shift)
    assert len(np.unique(row)) == VCB
    return _check(row)


def first_max(ids, seed):
    """the maximum at every id of `ids`, everything else lower (N(0, 1) below it by >= 1)"""
    rng = np.random.default_rng(seed)
    row = rng.standard_normal(VCB).astype(np.float32)
    row[np.array(ids)] = np.float32(float(row.max()) + 1.0)
    return _check(row)


def peaked(i, seed):
    """id i 200 above the rest: at T = 0.01 every other p underflows to 0"""
    rng = np.random.default_rng(seed)
    row = (0.1 * rng.standard_normal(VCB)).astype(np.float32)
    row[i] = np.float32(float(row.max()) + 200.0)
    return _check(row)


def top_tied(ids):
    """`ids` tied on top, everything else at FAR"""
    row = np.full(VCB, FAR, np.float32)
    row[np.array(ids)] = 3.0
    return _check(row)


# ---------------------------------------------------------------- the files' rows
# One file carries eight rows, one per codebook.
SOURCES = ("small", "q8", "q4", "f16", "moved")
EOS = BOS + 1
# wave boundaries of the split pick, three wave ranges, beside the masked ids, a 64-id row boundary, and
# one lane holding the maximum in three of its rows (326 and 454 in wave 0's rows 5 and 7, 1286 in wave 2's)
FIRST_MAX_IDS = [(511, 512), (1023, 1024), (1535, 1536), (70, 700, 1500), (2015, EOS), (63, 64), (326, 454, 1286), (1023, 1024)]
_files = {}


def rows_of(name):
    """([8][VCB] f32, [8] pattern names) of a crafted file"""
    if name in _files:
        return _files[name]
    if name == "kedge":  # the k and T sweeps
        rows = [flat(1.25), gauss(11), gauss(12, positives=40), two_level(3, 13)[0], flat(-2.5), gauss(15, shift=-20.0),
                two_level(70, 16)[0], flat(0.75)]
        pats = ["flat", "gauss", "gauss_neg", "two_level3", "flat", "gauss_allneg", "two_level70", "flat"]
    elif name == "straddle":  # codebooks 0..3 built for k = 64, 4..7 for k = 80
        rows = [straddle(64, 20 + c)[0] for c in range(4)] + [straddle(80, 20 + c)[0] for c in range(4, 8)]
        pats = ["straddle64"] * 4 + ["straddle80"] * 4
    elif name in ("firstmax_a", "firstmax_b"):  # b: a's rows moved on by 3, (2015, EOS) in codebook 7
        sh = 0 if name == "firstmax_a" else 3
        rows = [first_max(FIRST_MAX_IDS[(c - sh) % 8], 30 + c) for c in range(8)]
        pats = ["first_max"] * 8
    elif name == "firstmax_eos":  # EOS alone the strict maximum of codebooks 5 and 7
        rows = [first_max((EOS,) if c in (5, 7) else FIRST_MAX_IDS[c], 40 + c) for c in range(8)]
        pats = ["first_max"] * 8
    elif name == "eos3":  # 5, 2015 and EOS tied on top of codebooks 2 and 7; the others peaked
        rows = [top_tied((5, 2015, EOS)) if c in (2, 7) else peaked((100, 1600, 0, 600, 2015, 3, 1100, 0)[c], 50 + c)
                for c in range(8)]
        pats = ["eos3" if c in (2, 7) else "peaked" for c in range(8)]
    elif name == "moved":  # the general per-row mask: specials at 1000 .. 1007 (row 15, lanes 40 .. 47), EOS 1001
        rows = [flat(1.25), two_level(70, 60, near=(999, 1008))[0], first_max((999, 1001), 61), first_max((1001, 1008), 62),
                two_level(3, 63, near=(1008,))[0], first_max((999, 1008), 64), gauss(65), first_max((999, 1001, 1008), 66)]
        pats = ["flat", "two_level70", "first_max", "first_max", "two_level3", "first_max", "gauss", "first_max"]
    else:
        raise KeyError(name)
    r = np.stack(rows).astype(np.float32)
    r.setflags(write=False)
    _files[name] = (r, pats)
    return _files[name]


def bos_of(name):
    return MOVED_BOS if name == "moved" else BOS


# the crafted files made from each source model
FILES_OF = {"small": ("kedge", "straddle", "firstmax_a", "firstmax_b", "firstmax_eos", "eos3"),
            "q8": ("kedge", "straddle", "firstmax_a", "firstmax_b", "firstmax_eos"), "q4": ("kedge", "straddle", "firstmax_a"),
            "f16": ("kedge", "straddle", "firstmax_a"), "moved": ("moved",)}
ALL_FILES = FILES_OF["small"] + FILES_OF["moved"]


def moved_source(ma):
    """the moved-ids model of tests/test_decode_gpu.py (audio_bos = 1000)"""
    cache = os.environ.get("MAGPIE_CACHE", "/tmp/magpie_amd_cache")
    os.makedirs(cache, exist_ok=True)
    return ma.synth_gguf(os.path.join(cache, f"magpie_small_bos{MOVED_BOS}_k32.gguf"), dec_layers=2, enc_layers=1,
                         lt_head_scale=ma.DECISIVE, audio_bos=MOVED_BOS)


def crafted(source_path, name):
    """The crafted file of rows_of(name) made from the cached synthetic GGUF `source_path`,
    written beside it (into $MAGPIE_CACHE); its name carries the rows' digest."""
    from gguf_raw import GgufRaw, _TYPE_BYTES
    rows, _ = rows_of(name)
    tag = hashlib.sha1(rows.tobytes()).hexdigest()[:10]
    stem = os.path.splitext(os.path.basename(source_path))[0]
    path = os.path.join(os.path.dirname(source_path), f"{stem}_pick_{name}_{tag}.gguf")
    if not os.path.exists(path):
        g = GgufRaw(source_path)
        buf = bytearray(g.buf)
        for c in range(8):
            ne, typ, off = g.tensors[f"local_transformer_out_projections.{c}.weight"]
            n = _TYPE_BYTES[typ](int(np.prod(ne)))  # zero bytes are zero in F32, F16, Q8_0 and Q4_0 storage
            buf[g.data + off:g.data + off + n] = bytes(n)
            ne, typ, off = g.tensors[f"local_transformer_out_projections.{c}.bias"]
            assert typ == 0 and [int(v) for v in ne] == [VCB], (ne, typ)
            buf[g.data + off:g.data + off + 4 * VCB] = rows[c].tobytes()
        tmp = f"{path}.tmp{os.getpid()}"
        with open(tmp, "wb") as f:
            f.write(buf)
        os.replace(tmp, path)
    return path


# ---------------------------------------------------------------- expectations
def masked(row, bos, forbid_eos):
    m = np.array(row, np.float32)
    for i in range(bos, bos + 8):
        if i != bos + 1 or forbid_eos:
            m[i] = -np.inf
    return m


def order(m, k, reverse=False):
    """the k candidates' ids in the contract's order: descending value, ties by ascending id
    (reverse: by descending id, the rule a wrong tie-break would follow)"""
    ids = np.arange(len(m))
    return np.lexsort((-ids if reverse else ids, -m.astype(np.float64)))[:min(k, len(m))]


def np_sample(m, T, k, u, reverse=False):
    """sample_top_k restated in numpy f32 (sequential float sums): (pick, its rank, the width of its interval).
    numpy's exp may differ from libm's expf in the last place; used only where the margin is
    far above that (the reversed-rule proof, the edges visited)."""
    o = order(m, k, reverse)
    with np.errstate(invalid="ignore"):
        p = np.exp((m[o] - m[o[0]]) / np.float32(T), dtype=np.float32)
    p = p / np.cumsum(p, dtype=np.float32)[-1]
    cum = np.cumsum(p, dtype=np.float32)
    hit = np.nonzero(np.float32(u) < cum)[0]
    r = int(hit[0]) if len(hit) else len(o) - 1
    return int(o[r]), r, float(p[r])


def decision_class(pattern, width):
    """flat / clear / dense of one decision (the header's margin rule): by the row's pattern and
    the width of the interval the draw fell in"""
    if pattern == "flat":
        return "flat"
    return "clear" if width >= DENSE else "dense"


def expected(orc, name, T, k, forbid_eos, seed, stream, step, scale=None):
    """(sampled[8], argmax[8], margin[8]) of one frame of file `name` from oracle.sample_top_k:
    the oracle's comparator (ties in ascending index) is the contract. The argmax is the
    k = 1 candidate; below the 0.01 threshold the pick is the argmax, margin inf. scale: under
    guidance, on cfg_mix of every row with itself (both branches of a crafted file hold the
    same logits)."""
    rows, _ = rows_of(name)
    smp, amx, mg = np.zeros(8, np.int32), np.zeros(8, np.int32), np.full(8, np.inf)
    for cb in range(8):
        row = rows[cb] if scale is None else cfg_mix(rows[cb], rows[cb], scale)
        m = masked(row, bos_of(name), forbid_eos)
        amx[cb] = smp[cb] = orc.sample_top_k(m, 1.0, 1, 0.0)[0]
        if np.float32(T) >= np.float32(0.01):
            smp[cb], mg[cb] = orc.sample_top_k(m, T, k, orc.draw_u(seed, stream, step, cb))
    return smp, amx, mg


_runs = {}


def expected_run(orc, name, T, k, ignore_eos, seed, stream, frames, scale=None):
    """The frames of a decode (codes [n][8], argmax, margins [n or n + 1][8], n_frames): EOS
    forbidden before frame 4, the run ends before the first frame whose sampled code or argmax
    is EOS in any codebook (the oracle's synthesize, simulated from the rows alone)."""
    key = (name, float(T), k, bool(ignore_eos), seed, stream, frames, scale)
    if key in _runs:
        return _runs[key]
    eos = bos_of(name) + 1
    codes, amax, margins = [], [], []
    for f in range(frames):
        s, a, g = expected(orc, name, T, k, ignore_eos or f < 4, seed, stream, f, scale)
        margins.append(g)
        if (s == eos).any() or (a == eos).any():
            break
        codes.append(s)
        amax.append(a)
    _runs[key] = {"codes": np.array(codes, np.int32).reshape(-1, 8), "amax": np.array(amax, np.int32).reshape(-1, 8),
                  "margins": np.array(margins), "n_frames": len(codes)}
    return _runs[key]


def cfg_mix(cond, uncond, scale):
    """csrc/mp_fused.hpp's cfg_mix in numpy f32: s * c + (1 - s) * u, each product and the sum
    rounded to f32 separately (no contraction)"""
    s = np.float32(scale)
    a = (s * np.asarray(cond, np.float32)).astype(np.float32)
    b = ((np.float32(1.0) - s).astype(np.float32) * np.asarray(uncond, np.float32)).astype(np.float32)
    return (a + b).astype(np.float32)


# ---------------------------------------------------------------- the case table
# (file, T, k, ignore_eos, seed, frames, what the draws of stream 0 must visit). Seeds were found
# once on the CPU (test_pick_edges_cpu.py holds what each was found for). visits, on the rows
# whose pattern the case is about:
#   first   a draw in the first candidate's interval
#   last    a draw in the k-th candidate's interval (k >= 2017: the last unmasked candidate's)
#   tie     draws at ranks k - 2 and k - 1: two members taken from the tie group at the k-th place
CASES = {}


def _case(cid, file, T, k, seed, frames=16, ignore_eos=True, about=(), visits=(), decisive=1):
    """decisive (the tie cases): how many decisions at least change under the reversed tie rules"""
    assert cid not in CASES
    CASES[cid] = dict(id=cid, file=file, T=T, k=k, ignore_eos=ignore_eos, seed=seed, frames=frames, about=tuple(about),
                      visits=tuple(visits), decisive=decisive)


# the first seed of 0, 1, .. that meets the case's conditions (0 where not listed)
SEEDS = {"k63": 11, "k65": 2, "k127": 2, "k128": 11, "k2015": 2967, "k2016": 2967, "k2017": 2967, "k2023": 2967, "k2024": 2967,
         "k64_T100": 8, "k65_T100": 11, "k128_T100": 8, "k2016_T100": 602, "k2017_T100": 602, "k2024_T100": 602,
         "T0.01_gauss": 2, "T100.0_gauss": 9, "T100.0_peaked": 5, "two_level70_k80": 968, "straddle_k64": 5380,
         "straddle_k80": 11465, "moved_k80": 29, "moved_k2016": 885}


def _seed(cid):
    return SEEDS.get(cid, 0)


def _build_table():
    for k in KS:  # each k against flat and gauss (and the two-level rows), T = 0.7
        vis = ("first", "last") if k > 1 else ("first",)
        _case(f"k{k}", "kedge", 0.7, k, _seed(f"k{k}"), about=("flat",), visits=vis)
    for k in (64, 65, 128, 129, 2016, 2017, 2024):  # and very flat: the k-th gauss candidate is reachable
        _case(f"k{k}_T100", "kedge", 100.0, k, _seed(f"k{k}_T100"), about=("flat", "gauss"), visits=("first", "last"))
    # each T against gauss and peaked. 0.0099 is greedy (no draw). At 0.01 and 0.7 the k-th of
    # 80 candidates of these rows holds p < 1e-20 (at 0.01: 0), which no 24-bit draw reaches:
    # the first candidate alone is asked for; at 100 both ends are.
    for T in TS:
        vis = () if T < 0.01 else ("first",) if T < 100.0 else ("first", "last")
        _case(f"T{T}_gauss", "kedge", T, 80, _seed(f"T{T}_gauss"), about=("gauss", "gauss_neg", "gauss_allneg"), visits=vis)
        _case(f"T{T}_peaked", "eos3", T, 80, _seed(f"T{T}_peaked"), about=("peaked",), visits=vis)
    _case("two_level3_k5", "kedge", 0.7, 5, _seed("two_level3_k5"), about=("two_level3",), visits=("first", "tie"))
    _case("two_level70_k80", "kedge", 0.7, 80, _seed("two_level70_k80"), about=("two_level70",), visits=("first", "tie"))
    _case("straddle_k64", "straddle", 0.7, 64, _seed("straddle_k64"), about=("straddle64",), visits=("first", "tie"), decisive=6)
    _case("straddle_k80", "straddle", 0.7, 80, _seed("straddle_k80"), about=("straddle80",), visits=("first", "tie"), decisive=6)
    for f in ("firstmax_a", "firstmax_b"):
        _case(f"{f}_greedy", f, 0.0, 80, 0, about=("first_max",))
        _case(f"{f}_greedy_eos_live", f, 0.0, 80, 0, ignore_eos=False, about=("first_max",))
        _case(f"{f}_k1", f, 0.7, 1, _seed(f"{f}_k1"), about=("first_max",))  # the rank-0 candidate among equals
        _case(f"{f}_k2", f, 0.7, 2, _seed(f"{f}_k2"), about=("first_max",), visits=("first", "last"))
    _case("firstmax_eos_stops", "firstmax_eos", 0.0, 80, 0, ignore_eos=False, about=("first_max",))
    _case("eos_sampled", "eos3", 0.7, 3, _seed("eos_sampled"), ignore_eos=False, about=("eos3",))
    for cid, T, k in (("moved_greedy", 0.0, 80), ("moved_k80", 0.7, 80), ("moved_k2016", 0.7, 2016)):
        _case(cid, "moved", T, k, _seed(cid), about=("flat", "two_level70", "two_level3", "first_max"),
              visits=("first", "last") if T else ())


TIE_CASES = ("two_level3_k5", "two_level70_k80", "straddle_k64", "straddle_k80", "firstmax_a_greedy", "firstmax_b_greedy",
             "firstmax_a_k1", "firstmax_b_k1", "firstmax_a_k2", "firstmax_b_k2", "moved_greedy", "moved_k80")
# the runs every mode takes (flat k = 80 and gauss k = 65 are decisions of T0.7_gauss and k65)
EVERYWHERE = ("T0.7_gauss", "k65", "straddle_k64", "straddle_k80", "two_level70_k80", "firstmax_a_greedy")
K_SWEEP = tuple(f"k{k}" for k in KS)
EOS_SAMPLED_STREAMS = (0, 1)  # eos_sampled's seed: the two streams stop on different frames, both >= 4
GUIDED = ("T0.7_gauss", "straddle_k64", "straddle_k80")  # flat, gauss; straddle
GUIDED_SCALES = (2.5, -0.5)


def about_cbs(case):
    pats = rows_of(case["file"])[1]
    return [c for c in range(8) if pats[c] in case["about"]]


def last_rank(case, cb, forbid_eos):
    """the rank a `last` visit must hit: k - 1, or the last unmasked candidate's"""
    m = masked(rows_of(case["file"])[0][cb], bos_of(case["file"]), forbid_eos)
    return min(case["k"], int(np.isfinite(m).sum())) - 1


def survey(orc, case, stream=0):
    """every decision of the case's own run on the CPU: per frame and codebook the pick's
    rank, margin and class; the visits; the minimum margin of the clear rows; the share of the
    dense rows' decisions under BAR"""
    rows, pats = rows_of(case["file"])
    run = expected_run(orc, case["file"], case["T"], case["k"], case["ignore_eos"], case["seed"], stream, case["frames"])
    sampling = np.float32(case["T"]) >= np.float32(0.01)
    out = {"run": run, "decisions": 8 * len(run["margins"]), "visited": set(), "min_clear": np.inf, "dense": 0, "dense_under": 0}
    if not sampling:
        return out
    ranks_hit = {}
    for f in range(len(run["margins"])):
        forbid = case["ignore_eos"] or f < 4
        for cb in range(8):
            m = masked(rows[cb], bos_of(case["file"]), forbid)
            u = orc.draw_u(case["seed"], stream, f, cb)
            pick, mg = orc.sample_top_k(m, case["T"], case["k"], u)
            pick_np, r, width = np_sample(m, case["T"], case["k"], u)
            assert pick_np == pick or mg < 1e-6, (case["id"], f, cb, pick, pick_np, mg)
            cls = decision_class(pats[cb], width)
            if cls == "clear":
                out["min_clear"] = min(out["min_clear"], mg)
            elif cls == "dense":
                out["dense"] += 1
                out["dense_under"] += mg < BAR
            if pats[cb] in case["about"] and pick_np == pick:
                ranks_hit.setdefault(cb, set()).add((r, r == last_rank(case, cb, forbid)))
    hit = [r for s in ranks_hit.values() for r in s]
    if any(r == 0 for r, _ in hit):
        out["visited"].add("first")
    if any(last for _, last in hit):
        out["visited"].add("last")
    if any({(case["k"] - 2), (case["k"] - 1)} <= {r for r, _ in s} for s in ranks_hit.values()):
        out["visited"].add("tie")
    return out


_build_table()
